// Weight gradient of the convolutions for gfx950 (MI355X): dW = dY^T * gather(X), the implicit-GEMM kernels; the tap-sharing
// kernel for k x k layers on large maps is conv_wgrad_taps.hip (interface: wgrad_taps.h).
//
//   * the reduction runs over pixels (K = N*OH*OW): both operands are k-strided in memory, so fragments come from LDS through
//     ds_read_b64_tr_b16 (hardware transpose read); 64-lane waves, v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulate;
//   * split-K over pixels.  Grouped launches (one per tile variant for all layers of a step, fn_conv2d_wgrad_grouped) are
//     deterministic and atomic-free: a split stores its tile into its own fp32 slab and wgrad_reduce_kernel adds the slabs in
//     order.  Only the single-layer launch (fn_conv2d_wgrad) still accumulates into dW with fp32 global atomics.
#include "conv_args.h"

namespace fn {

// ------------------------------------------------------------------------------------------------
// wgrad: dW[co][kcol] += sum_m dY[m][co] * X[m @ tap(kcol)][ci(kcol)]
// ------------------------------------------------------------------------------------------------
// k-step pixel permutation shared by both operands: tile row of MFMA k index (g = lane>>4, h = half, q)
//   rho = q + 4*(g&1) + 8*h + 16*(g>>1)   -> the 8 rows a 32-lane half reads per ds_read_b64_tr_b16
//   are distinct mod 8, which with row strides of 160 B / 288 B makes the transposed reads conflict free.
template <typename T, int BMW, int BNW, bool NORM>
__device__ __forceinline__ void conv_wgrad_body(const WgradArgs& a, const int bx, const int by, const int bz) {
    constexpr int BK = 64;                   // pixels per stage
    constexpr int DEPTH = (BMW * BNW <= 64 * 64) ? 3 : (BMW * BNW <= 64 * 128 ? 2 : 1);   // register stages in flight
    constexpr int RSA = BMW * 2 + 32;        // LDS row strides in bytes (160 for 64, 288 for 128, 96 for 32)
    constexpr int RSB = BNW * 2 + 32;
    constexpr int A_BYTES = BK * RSA, B_BYTES = BK * RSB;
    constexpr int CGA = BMW / 8, CGB = BNW / 8;  // 16-B chunks per row
    constexpr int AP = BK * CGA / 256, BP = BK * CGB / 256;
    constexpr int WMW = (BMW >= 64) ? 2 : 1, WNW = 4 / WMW;
    constexpr int TM = BMW / WMW, TN = BNW / WNW;
    constexpr int MREP = TM / 16, NREP = TN / 16;
    static_assert(AP >= 1 && BP >= 1 && MREP >= 1 && NREP >= 1, "tile too small");
    typedef typename LP<T>::vec8 vec8;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;                 // [2][BK][RSA]  dY tile  (rows = pixels, cols = co)
    unsigned char* sB = smem + 2 * A_BYTES;   // [2][BK][RSB]  X  tile  (rows = pixels, cols = kcol)
    float* sNs = reinterpret_cast<float*>(smem + 2 * (A_BYTES + B_BYTES));   // NORM: [BNW] scale, [BNW] shift of this tile's columns
    float* sNh = sNs + BNW;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const int n0 = bx * BNW;  // kcol tile
    const int c0 = by * BMW;  // cout tile
    const int mbeg = bz * a.chunk;
    const int mend = min(a.M, mbeg + a.chunk);
    const int nst = (mend - mbeg + BK - 1) / BK;
    if (nst <= 0) return;
    if constexpr (NORM) {
        if (tid < BNW) {
            const int e = ktab_entry((n0 >> 3) + (tid >> 3), a.KTOT, a.Cin, a.KW);
            float sc = 0.f, sh = 0.f, mean, var;
            if (e >= 0) {
                const int c = (e & 0xffff) + (tid & 7);
                bn_batch_affine(a.nrm_stats, c, a.nrm_sq_off, a.nrm_replicas, a.nrm_rep_stride, a.nrm_count, a.nrm_eps, a.nrm_beta[c], sc, sh,
                                mean, var);
            }
            sNs[tid] = sc;
            sNh[tid] = sh;
        }
        __syncthreads();
    }

    // B-operand columns handled by this thread (fixed for the whole kernel)
    int bcol_c[BP], bcol_dy[BP], bcol_dx[BP], brow[BP];
    bool bcol_ok[BP];
#pragma unroll
    for (int j = 0; j < BP; ++j) {
        const int cidx = tid + 256 * j;
        brow[j] = cidx / CGB;
        const int e = ktab_entry((n0 >> 3) + (cidx % CGB), a.KTOT, a.Cin, a.KW);
        bcol_ok[j] = e >= 0;
        bcol_dy[j] = ((e >> 24) & 0xff) - a.pad_h;
        bcol_dx[j] = ((e >> 16) & 0xff) - a.pad_w;
        bcol_c[j] = e & 0xffff;
    }
    int arow[AP], acol[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        const int cidx = tid + 256 * i;
        arow[i] = cidx / CGA;
        acol[i] = c0 + (cidx % CGA) * 8;
    }

    u32x4 ra[DEPTH][AP], rb[DEPTH][BP];
    unsigned bmask[DEPTH];   // NORM only: X chunks of a stage that hold real pixels (bits 8..)
    // buffer loads with hardware zero fill (see conv_igemm_body): ragged rows / columns and padding need no select
    constexpr unsigned OOB = 0x60000000u;
    const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.dy), 0, a.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.x), 0, a.x_bytes, 0x00020000);
    unsigned acolb[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) acolb[i] = acol[i] < a.Cout ? (unsigned)acol[i] * 2u : OOB;
    auto load_tile = [&](int stg, u32x4 (&ra)[AP], u32x4 (&rb)[BP], unsigned& msk) {
        unsigned mk = 0u;
        const int mb = mbeg + stg * BK;
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const int m = mb + arow[i];
            const unsigned off = m < mend ? (unsigned)m * (unsigned)a.ld_y * 2u + acolb[i] : OOB;
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_dy, (int)off, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) {
            const int m = mb + brow[j];
            bool ok = m < mend && bcol_ok[j];
            int pix = m;
            if (!a.plain) {
                int n, rem, oy, ox;
                fast_divmod(m, a.OH * a.OW, a.inv_ohw, n, rem);
                fast_divmod(rem, a.OW, a.inv_ow, oy, ox);
                const int iy = oy * a.stride + bcol_dy[j], ix = ox * a.stride + bcol_dx[j];
                ok = ok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                pix = (n * a.H + iy) * a.W + ix;
            }
            const unsigned off = ok ? ((unsigned)pix * (unsigned)a.ld_x + (unsigned)bcol_c[j]) * 2u : OOB;
            rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)off, 0, 0);
            if constexpr (NORM) mk |= (ok ? 1u : 0u) << (8 + j);
        }
        msk = mk;
    };
    auto store_tile = [&](int buf, const u32x4 (&ra)[AP], const u32x4 (&rb)[BP], const unsigned msk) {
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const int cidx = tid + 256 * i;
            *reinterpret_cast<u32x4*>(sA + buf * A_BYTES + arow[i] * RSA + (cidx % CGA) * 16) = ra[i];
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) {
            const int cidx = tid + 256 * j;
            u32x4 v = rb[j];
            if constexpr (NORM) {
                if (msk & (1u << (8 + j))) {
                    const int col = (cidx % CGB) * 8;
                    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sNs + col), s1 = *reinterpret_cast<const f32x4*>(sNs + col + 4);
                    const f32x4 h0 = *reinterpret_cast<const f32x4*>(sNh + col), h1 = *reinterpret_cast<const f32x4*>(sNh + col + 4);
                    float f[8];
                    unpack8<T>(v, f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        f[e] = fmaxf(fmaf(f[e], s0[e], h0[e]), 0.f);
                        f[4 + e] = fmaxf(fmaf(f[4 + e], s1[e], h1[e]), 0.f);
                    }
                    v = pack8<T>(f);
                }
            }
            *reinterpret_cast<u32x4*>(sB + buf * B_BYTES + brow[j] * RSB + (cidx % CGB) * 16) = v;
        }
    };

    f32x4 acc[MREP][NREP];
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read addressing: lane -> (g, q, p); supplies the address of row rho(g,h,q), columns 4p..4p+3
    const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
    const int rho0 = q + 4 * (g & 1) + 16 * (g >> 1);  // + 8*h + 32*ks
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
    auto compute = [&](int buf) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            vec8 fa[MREP], fb[NREP];
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                const unsigned char* base = sA + buf * A_BYTES + (wm * TM + i * 16 + 4 * p) * 2;
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + (rho0 + 32 * ks) * RSA));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + (rho0 + 8 + 32 * ks) * RSA));
                fa[i] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                const unsigned char* base = sB + buf * B_BYTES + (wn * TN + j * 16 + 4 * p) * 2;
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + (rho0 + 32 * ks) * RSB));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + (rho0 + 8 + 32 * ks) * RSB));
                fb[j] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int i = 0; i < MREP; ++i)
#pragma unroll
                for (int j = 0; j < NREP; ++j) acc[i][j] = LP<T>::mfma(fa[i], fb[j], acc[i][j]);
        }
    };

    const int last = nst - 1;   // branch-free steady state, clamped stage index (see conv_igemm_body)
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load_tile(min(d, last), ra[d], rb[d], bmask[d]);
    store_tile(0, ra[0], rb[0], bmask[0]);
    __syncthreads();
    for (int s0 = 0; s0 < nst; s0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int stg = s0 + d;
            load_tile(min(stg + DEPTH, last), ra[d], rb[d], bmask[d]);
            if (stg < nst) compute(stg & 1);
            store_tile((stg + 1) & 1, ra[(d + 1) % DEPTH], rb[(d + 1) % DEPTH], bmask[(d + 1) % DEPTH]);
            __syncthreads();
        }
    }

    // C layout: col = lane&15 (kcol), row = (lane>>4)*4 + r (cout)
    float* const dst = a.out.ws ? a.out.ws + (long)bz * a.Cout * a.KTOT : a.dw;
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            const int kc = n0 + wn * TN + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = c0 + wm * TM + i * 16 + g * 4 + r;
                if (co < a.Cout && kc < a.KTOT) {
                    if (a.out.store) dst[(long)co * a.KTOT + kc] = acc[i][j][r];
                    else unsafeAtomicAdd(&a.dw[(long)co * a.KTOT + kc], acc[i][j][r]);
                }
            }
        }
}

// Second stage of the grouped weight gradients: dw = slab 0 + slab 1 + ... in that order (blockIdx.y = layer; the per-layer
// records of either weight-gradient kernel start with a WgradOut and are `stride` bytes apart).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const unsigned char* __restrict__ args, int stride) {
    const WgradOut a = *reinterpret_cast<const WgradOut*>(args + (long)blockIdx.y * stride);
    if (a.ws == nullptr) return;
    const long n4 = (long)a.Cout * a.KTOT / 4;          // layer sizes are multiples of 4
    const f32x4* ws = reinterpret_cast<const f32x4*>(a.ws);
    f32x4* dw = reinterpret_cast<f32x4*>(a.dw);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 s = ws[i];
        int z = 1;
        for (; z + 8 <= a.splits; z += 8) {       // eight slab reads in flight, added in slab order
            f32x4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = ws[(long)(z + k) * n4 + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; z < a.splits; ++z) s += ws[(long)z * n4 + i];
        dw[i] = s;
    }
}

template <typename T, int BMW, int BNW, bool NORM>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
    conv_wgrad_body<T, BMW, BNW, NORM>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Grouped form: ONE launch computes the weight gradients of many layers.  Weight gradients have no consumer before the
// optimiser, so the engine defers them to the end of backward and issues them per tile configuration: thousands of
// workgroups per launch instead of 133 launches that each fill a fraction of the 256 CUs.
// args[g] describes layer g; prefix[g] .. prefix[g+1] are its workgroups (gx * gy * splits).
template <typename T, int BMW, int BNW, bool NORM>
__global__ __launch_bounds__(256) void conv_wgrad_grouped_kernel(const unsigned char* __restrict__ args_raw, int stride, const int* __restrict__ prefix, int n) {
    const int bid = blockIdx.x;
    int lo = 0, hi = n;                    // largest g with prefix[g] <= bid
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= bid) lo = mid; else hi = mid;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);           // wave-uniform: scalar loads of the record
    const WgradArgs a = *reinterpret_cast<const WgradArgs*>(args_raw + (long)lo * stride);
    // Workgroups that share a pixel chunk (same split, all gx*gy tiles) are consecutive in the layer's logical order: inside
    // the layer give every XCD a contiguous run of it, so a chunk of X / dY is fetched into one L2 instead of all eight
    // (per layer, not per launch: whole layers on one XCD would unbalance the chip).
    const int gxy = a.gx * a.gy;
    const int local = xcd_remap(bid - prefix[lo], gxy * a.splits);
    const int bz = local / gxy, r = local - bz * gxy;
    conv_wgrad_body<T, BMW, BNW, NORM>(a, r % a.gx, r / a.gx, bz);
}

// the BMW x BNW tiles both weight-gradient kernels are instantiated for
#define FN_WGRAD_TILES(X) X(32, 64) X(32, 128) X(64, 64) X(64, 128) X(128, 64) X(128, 128)

// Dynamic LDS of a workgroup: two stages of 64 pixel rows of both operands (row strides BMW * 2 + 32 and BNW * 2 + 32 bytes; 64x64
// stages are exactly 40 KiB: four workgroups per CU).  Only normalise-on-load launches pay for the affine table.
static size_t wgrad_smem_bytes(int bmw, int bnw, bool norm) {
    return (size_t)2 * 64 * ((bmw * 2 + 32) + (bnw * 2 + 32)) + (norm ? 2 * bnw * 4 : 0);
}

template <typename T, int BMW, int BNW> static int launch_wgrad(const WgradArgs& a, int splits, hipStream_t st) {
    const size_t smem = wgrad_smem_bytes(BMW, BNW, a.nrm_stats != nullptr);
    dim3 grid(cdiv(a.KTOT, BNW), cdiv(a.Cout, BMW), splits);
    if (a.nrm_stats) hipLaunchKernelGGL((conv_wgrad_kernel<T, BMW, BNW, true>), grid, dim3(256), smem, st, a);
    else hipLaunchKernelGGL((conv_wgrad_kernel<T, BMW, BNW, false>), grid, dim3(256), smem, st, a);
    return check_launch("conv_wgrad");
}

static void choose_wgrad_tile(int Cout, int KTOT, int& bmw, int& bnw) {
    bmw = Cout <= 32 ? 32 : (Cout <= 64 || Cout % 128 != 0 ? 64 : 128);
    bnw = (KTOT <= 64 || (cdiv(KTOT, 128) * 128 - KTOT) > 32) ? 64 : 128;
}

// Split-K factor over pixels, modelled on the single-layer launch (fn_conv2d_wgrad), where every split adds one fp32 copy of dW
// through global atomics (~1.3 TB/s chip-wide, MI355X_MICROARCH.md) while fewer splits mean a longer serial stage chain per
// workgroup (~0.5 us per 64-pixel stage at the occupancy these launches get).  Minimise  stages(s)*0.5us + s*bytes(dW)/1.3TB/s
// subject to filling the chip.  Grouped launches start from the same number and cap it in plan_wgrad(): their splits cost a
// slab store and a share of the ordered reduction instead of atomics.
static int choose_wgrad_splits(int M, int Cout, int KTOT, int bmw, int bnw) {
    const long tiles = (long)cdiv(KTOT, bnw) * cdiv(Cout, bmw);
    const int stages = cdiv(M, 64);
    static const int stem_wgs = env_int("FN_WG_STEMWGS", 1024);   // tuning aid
    if (stages >= 1024) {   // long chains (stem): ~1024 workgroups in total, at least 4 stages each
        int s = (int)((stem_wgs + tiles - 1) / tiles);
        if (s > stages / 4) s = stages / 4;
        return s < 1 ? 1 : s;
    }
    const double atom_us = (double)Cout * KTOT * 4.0 / 1.3e6;   // one fp32 copy of dW
    int best = 1;
    double best_t = 1e30;
    for (int s = 1; s <= stages && s <= 512; s = (s < 8 ? s + 1 : s + s / 4)) {
        const double waves = (double)(tiles * s) / 512.0;        // ~2 workgroups per CU resident
        const double t = cdiv(stages, s) * 0.5 * (waves > 1.0 ? waves : 1.0) + s * atom_us;
        if (t < best_t) { best_t = t; best = s; }
    }
    return best;
}

static void final_wgrad_tile(int Cout, int KTOT, int& bmw, int& bnw) {
    choose_wgrad_tile(Cout, KTOT, bmw, bnw);
    static const int big = env_int("FN_WGRAD_BIG", 0);   // tuning aid
    if (big == 1) return;
    // small problems: prefer 64-wide tiles so that enough workgroups exist without a deep split
    if ((long)cdiv(KTOT, bnw) * cdiv(Cout, bmw) < (big == 2 ? 16 : 64)) {
        if (bmw == 128) bmw = 64;
        if (bnw == 128 && KTOT > 64) bnw = 64;
    }
}

static int plan_wgrad(WgradArgs& a, int want_splits, int bmw, int bnw, bool grouped) {
    int splits = want_splits > 0 ? want_splits : choose_wgrad_splits(a.M, a.Cout, a.KTOT, bmw, bnw);
    if (grouped && want_splits <= 0) {
        // inside a grouped launch the chip is full anyway: fewer, longer splits.  Every split adds one fp32 copy of dW -- its slab,
        // stored and then read again by wgrad_reduce_kernel -- and that traffic, not the MFMA work, is what the launch is made of
        // once X / dY come from L2: measured 606 / 533 / 510 / 502 / 504 / 591 us for >= 8 / 16 / 32 / 48 / 64 / 96 stages per split
        static const int min_stages = env_int("FN_WG_MINSTAGES", 48);   // tuning aid
        const int cap = cdiv(cdiv(a.M, 64), min_stages);
        if (splits > cap) splits = cap < 1 ? 1 : cap;
    }
    a.chunk = cdiv(cdiv(a.M, splits), 64) * 64;
    splits = cdiv(a.M, a.chunk);
    a.gx = cdiv(a.KTOT, bnw);
    a.gy = cdiv(a.Cout, bmw);
    a.splits = splits;
    return splits;
}

template <typename T> static int dispatch_wgrad(WgradArgs& a, int want_splits, hipStream_t st) {
    int bmw, bnw;
    final_wgrad_tile(a.Cout, a.KTOT, bmw, bnw);
    const int splits = plan_wgrad(a, want_splits, bmw, bnw, false);
#define FN_X(BM_, BN_) \
    if (bmw == BM_ && bnw == BN_) return launch_wgrad<T, BM_, BN_>(a, splits, st);
    FN_WGRAD_TILES(FN_X)
#undef FN_X
    set_error("conv_wgrad: no tile %dx%d", bmw, bnw);
    return FN_EUNSUPPORTED;
}

int wgrad_variant(const fn_conv_desc* d) {
    if (const int tv = wgrad_taps_variant(d)) return tv;     // k x k layers on maps of >= 32 pixels: the tap-sharing kernel
    int bmw, bnw;
    final_wgrad_tile(d->Cout, d->KH * d->KW * d->Cin, bmw, bnw);
    return wgrad_variant_encode(bmw, bnw, false);            // callers add the flag of a normalise-on-load group themselves
}

}  // namespace fn

using namespace fn;

static int make_wgrad_args(const fn_conv_desc* d, WgradArgs& a) {
    if (int rc = check_desc(d)) return rc;
    FN_REQUIRE(d->x && d->y && d->dw, "conv_wgrad: null x/dy/dw");
    FN_REQUIRE(d->ld_y % 8 == 0 && d->ld_y >= d->Cout, "conv_wgrad: ld_y=%d invalid", d->ld_y);
    FN_REQUIRE((long)d->N * d->OH * d->OW < (1L << 24), "conv_wgrad: N*OH*OW must be < 2^24");
    a = WgradArgs{};
    a.x = (const unsigned short*)d->x; a.dy = (const unsigned short*)d->y; a.dw = d->dw;
    a.M = d->N * d->OH * d->OW; a.OH = d->OH; a.OW = d->OW; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.KTOT = d->KH * d->KW * d->Cin; a.KW = d->KW; a.stride = d->stride; a.pad_h = d->pad_h; a.pad_w = d->pad_w;
    a.ld_x = d->ld_x; a.ld_y = d->ld_y;
    a.plain = is_plain(d);
    a.inv_ow = 1.0f / (float)d->OW; a.inv_ohw = 1.0f / (float)(d->OH * d->OW);
    FN_REQUIRE((long)d->N * d->H * d->W * d->ld_x * 2 < (1L << 30) && (long)a.M * d->ld_y * 2 < (1L << 30),
               "conv_wgrad: x or dy exceeds the 1 GiB range of 32-bit buffer offsets");
    a.x_bytes = d->N * d->H * d->W * d->ld_x * 2;
    a.dy_bytes = a.M * d->ld_y * 2;
    if (d->nrm_stats) {
        FN_REQUIRE(d->nrm_beta && d->nrm_count > 0 && d->nrm_eps > 0.f, "conv_wgrad: normalise-on-load needs beta, count, eps");
        copy_norm_fields(d, a);
    }
    return FN_OK;
}

extern "C" int fn_conv2d_wgrad(const fn_conv_desc* d, void* stream) {
    WgradArgs a;
    if (int rc = make_wgrad_args(d, a)) return rc;
    return d->dtype == FN_BF16 ? dispatch_wgrad<__bf16>(a, d->splits, (hipStream_t)stream)
                               : dispatch_wgrad<_Float16>(a, d->splits, (hipStream_t)stream);
}

// ---- grouped weight gradients ------------------------------------------------------------------------------------
// one record size for both weight-gradient kernels (groups of either kind use the same host / device buffers)
extern "C" int fn_conv2d_wgrad_arg_bytes(void) {
    const size_t a = sizeof(WgradArgs), b = wgrad_taps_arg_bytes();
    return (int)(((a > b ? a : b) + 15) / 16 * 16);
}

// Host-side planning: fills host_args[n * fn_conv2d_wgrad_arg_bytes()] and host_prefix[n+1] for n descriptors that all
// dispatch to `variant` (= fn_conv2d_variant(desc, 2)); returns the total number of workgroups (or a negative status).
extern "C" int fn_conv2d_wgrad_group_build(const fn_conv_desc* descs, int n, int variant, void* host_args, int32_t* host_prefix, float* ws,
                                           int64_t* ws_elems) {
    FN_REQUIRE(descs && host_args && host_prefix && ws_elems && n > 0, "wgrad_group_build: bad arguments");
    long ws_used = 0;
    const size_t rec_bytes = (size_t)fn_conv2d_wgrad_arg_bytes();
    if (variant >= WGRAD_TAPS_VARIANT) {      // tap-sharing kernel (conv_wgrad_taps.hip)
        long total = 0;
        for (int i = 0; i < n; ++i) {
            if (int rc = check_desc(&descs[i])) return rc;
            FN_REQUIRE(descs[i].dtype == descs[0].dtype, "wgrad_group_build: mixed dtypes");
            host_prefix[i] = (int32_t)total;
            const long wgs = wgrad_taps_plan(&descs[i], variant, reinterpret_cast<unsigned char*>(host_args) + i * rec_bytes, ws, &ws_used);
            if (wgs < 0) return (int)wgs;
            total += wgs;
        }
        FN_REQUIRE(total < (1L << 30), "wgrad_group_build: too many workgroups");
        host_prefix[n] = (int32_t)total;
        *ws_elems = ws_used;
        return (int)total;
    }
    int bmw, bnw;
    bool norm;
    wgrad_variant_decode(variant, bmw, bnw, norm);
    long total = 0;
    for (int i = 0; i < n; ++i) {
        WgradArgs a;
        if (int rc = make_wgrad_args(&descs[i], a)) return rc;
        int m, k;
        final_wgrad_tile(a.Cout, a.KTOT, m, k);
        FN_REQUIRE(m == bmw && k == bnw, "wgrad_group_build: descriptor %d dispatches to %dx%d, group is %dx%d", i, m, k, bmw, bnw);
        FN_REQUIRE(descs[i].dtype == descs[0].dtype, "wgrad_group_build: mixed dtypes");
        FN_REQUIRE((a.nrm_stats != nullptr) == norm, "wgrad_group_build: descriptor %d: normalise-on-load members need a group of their own (variant + 1000000)", i);
        const int splits = plan_wgrad(a, descs[i].splits, bmw, bnw, true);
        FN_REQUIRE(((long)a.Cout * a.KTOT) % 4 == 0, "wgrad_group_build: descriptor %d: Cout*K must be a multiple of 4", i);
        a.out = WgradOut{a.dw, nullptr, a.Cout, a.KTOT, splits, 1};
        if (splits > 1) {            // slabs of this layer: [splits][Cout*KTOT]; ws == NULL on the sizing call
            a.out.ws = ws ? ws + ws_used : reinterpret_cast<float*>(16);
            ws_used += (long)splits * a.Cout * a.KTOT;
        }
        host_prefix[i] = (int32_t)total;
        total += (long)a.gx * a.gy * splits;
        *reinterpret_cast<WgradArgs*>(reinterpret_cast<unsigned char*>(host_args) + i * rec_bytes) = a;
    }
    FN_REQUIRE(total < (1L << 30), "wgrad_group_build: too many workgroups");
    host_prefix[n] = (int32_t)total;
    *ws_elems = ws_used;
    return (int)total;
}

extern "C" int fn_conv2d_wgrad_reduce(const void* dev_args, int n, void* stream) {
    FN_REQUIRE(dev_args && n > 0 && n < 65536, "wgrad_reduce: bad arguments");
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(64, n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned char*>(dev_args),
                       fn_conv2d_wgrad_arg_bytes());
    return check_launch("wgrad_reduce");
}

template <typename T> static int launch_wgrad_grouped(const void* args, const int32_t* prefix, int n, int total, int variant, hipStream_t st) {
    int bmw, bnw;
    bool norm;      // every member normalises x on load
    wgrad_variant_decode(variant, bmw, bnw, norm);
    const unsigned char* a = reinterpret_cast<const unsigned char*>(args);
    const int stride_ = fn_conv2d_wgrad_arg_bytes();
#define FN_X(BM_, BN_)                                                                                                      \
    if (bmw == BM_ && bnw == BN_) {                                                                                         \
        const size_t sm_ = wgrad_smem_bytes(BM_, BN_, norm);                                                                \
        if (norm) hipLaunchKernelGGL((conv_wgrad_grouped_kernel<T, BM_, BN_, true>), dim3(total), dim3(256), sm_, st, a, stride_, prefix, n); \
        else hipLaunchKernelGGL((conv_wgrad_grouped_kernel<T, BM_, BN_, false>), dim3(total), dim3(256), sm_, st, a, stride_, prefix, n);    \
        return check_launch("conv_wgrad_grouped");                                                                          \
    }
    FN_WGRAD_TILES(FN_X)
#undef FN_X
    set_error("wgrad_grouped: unknown variant %d", variant);
    return FN_EINVAL;
}

extern "C" int fn_conv2d_wgrad_grouped(const void* dev_args, const int32_t* dev_prefix, int n, int total_blocks, int variant, int dtype,
                                       void* stream) {
    FN_REQUIRE(dev_args && dev_prefix && n > 0 && total_blocks > 0, "wgrad_grouped: bad arguments");
    FN_REQUIRE(dtype == FN_BF16 || dtype == FN_F16, "dtype %d unsupported", dtype);
    if (variant >= WGRAD_TAPS_VARIANT) return wgrad_taps_launch(dev_args, dev_prefix, n, total_blocks, variant, dtype, (hipStream_t)stream);
    return dtype == FN_BF16 ? launch_wgrad_grouped<__bf16>(dev_args, dev_prefix, n, total_blocks, variant, (hipStream_t)stream)
                            : launch_wgrad_grouped<_Float16>(dev_args, dev_prefix, n, total_blocks, variant, (hipStream_t)stream);
}
