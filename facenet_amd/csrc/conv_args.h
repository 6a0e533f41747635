// Argument records of the convolution kernels and what conv_igemm.hip (forward / data gradient) and conv_wgrad.hip (weight
// gradient) share.  The records are copied to the device byte for byte: layout and field order are part of the kernels.
#pragma once
#include "common.h"
#include "../../include/facenet_hip.h"
#include "wgrad_taps.h"

namespace fn {

struct ConvArgs {
    const unsigned short* src;  // gathered activation operand
    const unsigned short* wp;   // packed weights [NOUT][KTOT]
    void* out;
    const float* bias;
    acc_t* stats;               // BatchNorm batch statistics (fixed point, ACC_STAT): stats[rep*stride + c] += sum y, [.. + sq_off + c] += sum y^2
    const unsigned short* resid;
    int M, PH, PW;   // output pixels = N*PH*PW
    int SH, SW;      // source spatial dims
    int CS;          // source channels per tap
    int NOUT, KTOT, KH, KW;
    int so, sk, offy, offx, dshift;  // t = p*so + k*sk + off ; src = t >> dshift, valid iff t>=0, (t & ((1<<dshift)-1))==0, src < S
    int ld_src, ld_out, ld_res;
    int relu, accumulate, out_f32;
    float scale;
    int tiles_m, tiles_n;
    int stats_sq_off, stats_replicas, stats_rep_stride;
    int plain;  // 1x1 / stride 1 / no padding: source pixel == output pixel, k == channel
    // dgrad epilogue: reduction of the BatchNorm backward of the layer whose output gradient this launch produces
    const unsigned short* bn_y;   // raw forward output of that layer (same pixels / channel slice as `out`)
    const float* bn_scale;
    const float* bn_shift;
    const float* bn_beta;
    acc_t* bn_acc;                // fixed point (ACC_GRAD): acc[rep*stride + c] += sum dyh ; acc[rep*stride + sq_off + c] += sum dyh*xhat
    int ld_bn_y, bn_sq_off, bn_replicas, bn_rep_stride, bn_relu;
    // stride-2 dgrad: output pixels are split into 4 parity classes ((iy+pad)&1, (ix+pad)&1); a class only sees the taps
    // of matching parity, so each class is its own GEMM (M = its pixels, K = its taps) inside one launch.
    int s2;                 // 1 = class mode
    int cp1, cp2, cp3;      // first tile of classes 1..3 (class 0 starts at 0)
    int total_tiles;
    int src_bytes, w_bytes;   // extents for the buffer resource descriptors (< 2^30)
    int tile;                 // 0 = heuristic, BM*1000+BN = caller's choice (fn_conv_desc.tile_fwd / tile_dgrad)
    int nocheck;              // forward, no padding: taps never leave the source, the per-chunk bounds test is skipped
    // 1x1 data gradient of SIBLING layers that read the same input: dX = sum_s dY_s * Wt_s as ONE GEMM whose K runs through
    // the sources (k tiles [0,t1) source 1, [t1,t2) source 2, [t2,nt_total) source 3); nt_total == 0: single source
    const unsigned short* src2; const unsigned short* wp2;
    const unsigned short* src3; const unsigned short* wp3;
    int K2, ld2, K3, ld3, t1, t2, nt_total, src2_bytes, w2_bytes, src3_bytes, w3_bytes;
    // normalise-on-load (forward only): src is the raw output of a BN(center)+ReLU layer, see fn_conv_desc.nrm_*
    const acc_t* nrm_stats;
    const float* nrm_beta;
    int nrm_sq_off, nrm_replicas, nrm_rep_stride, nrm_count;
    float nrm_eps;
    unsigned short* nrm_z;    // optional: the normalised operand is also written here (geometry of src), see fn_conv_desc.nrm_z
    // dgrad epilogue: fused residual backward (fn_conv_desc.rb_*).  `resid` (scale 1) carries rb_prev, `out` is rb_dtrunk.
    int halo_ty, halo_tx;         // halo kernel: 8x16-pixel output tiles per image (rows, columns)
    const unsigned short* mask;   // rows of the block's forward output: values <= 0 zero the gradient
    unsigned short* out2;         // scale2 * (masked gradient), geometry of out
    acc_t* colsum;                // fixed point (ACC_GRAD): += column sums of what goes to out2
    float scale2;
    const float* prelu;           // forward: per-output-channel PReLU slope applied to conv + bias
};

struct WgradArgs {
    WgradOut out;   // first member: where the result goes (grouped launches; wgrad_reduce_kernel reads it through a byte stride)
    const unsigned short* x;
    const unsigned short* dy;
    float* dw;
    int M, OH, OW, H, W, Cin, Cout, KTOT, KW;
    int stride, pad_h, pad_w;
    int ld_x, ld_y;
    int chunk;  // pixels per split (multiple of 64)
    int gx, gy, splits;  // grid of this layer inside a grouped launch
    int plain;  // 1x1 stride-1: source pixel == output pixel
    float inv_ow, inv_ohw;
    int x_bytes, dy_bytes;   // extents for the buffer resource descriptors (< 2^30)
    // normalise-on-load of x (see fn_conv_desc.nrm_*)
    const acc_t* nrm_stats;
    const float* nrm_beta;
    int nrm_sq_off, nrm_replicas, nrm_rep_stride, nrm_count;
    float nrm_eps;
    // Grouped launches are DETERMINISTIC and atomic-free (out.store = 1): a layer with one split stores its tiles straight into
    // dw; a layer with several splits stores split z into slab z of out.ws and wgrad_reduce_kernel adds the slabs in order.
    // (Global float atomics run at ~1.3 TB/s at the memory side, plain stores at ~6 TB/s, and the order of atomic adds -- hence
    // the rounding of dW -- changed from run to run.)  out.store = 0: legacy single launch, atomic accumulation into dw.
};

// q = m / d, r = m % d through the hardware reciprocal (0 <= m < 2^24, d > 0): integer division is a ~40-instruction
// sequence on this ISA and the prologue of every workgroup needs several
__device__ __forceinline__ void rcp_divmod(int m, int d, int& q, int& r) { fast_divmod(m, d, __builtin_amdgcn_rcpf((float)d), q, r); }

__device__ __forceinline__ int ktab_entry(int kgroup, int KTOT, int CS, int KW) {
    const int k = kgroup * 8;
    if (k >= KTOT) return -1;
    int tap, c, ky, kx;
    rcp_divmod(k, CS, tap, c);
    rcp_divmod(tap, KW, ky, kx);
    return (ky << 24) | (kx << 16) | c;
}

// ---- host side, shared by the two translation units -----------------------------------------------------------------------------
int check_desc(const fn_conv_desc* d);          // geometry checks common to every operation (conv_igemm.hip)
int wgrad_variant(const fn_conv_desc* d);       // the weight-gradient half of fn_conv2d_variant (conv_wgrad.hip)

// 1x1 / stride 1 / no padding: source pixel == output pixel, k == channel
inline int is_plain(const fn_conv_desc* d) { return (d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad_h == 0 && d->pad_w == 0) ? 1 : 0; }

// normalise-on-load operand (fn_conv_desc.nrm_*) of a ConvArgs or WgradArgs record; the caller has checked what its kernel needs
template <typename Args> inline void copy_norm_fields(const fn_conv_desc* d, Args& a) {
    a.nrm_stats = d->nrm_stats; a.nrm_beta = d->nrm_beta; a.nrm_sq_off = d->nrm_sq_off;
    a.nrm_replicas = d->nrm_replicas > 0 ? d->nrm_replicas : 1; a.nrm_rep_stride = d->nrm_rep_stride;
    a.nrm_count = d->nrm_count; a.nrm_eps = d->nrm_eps;
}

// fn_conv2d_variant codes (include/facenet_hip.h; facenet_amd/_lib.py and bench.py decode them too):
//   forward / data gradient: BM * 1000 + BN (+ KS * 1000000 when the launch splits K, KS > 1); 9000000 + BN: the halo-tile kernel
//   weight gradient:         BMW * 1000 + BNW (+ 1000000 for a group whose members normalise x on load); from 5000000: wgrad_taps.h
enum { VARIANT_FLAG = 1000000, VARIANT_HALO = 9000000 };
inline int variant_encode(int bm, int bn, int ks) { return bm * 1000 + bn + (ks > 1 ? ks * VARIANT_FLAG : 0); }
inline void variant_decode(int code, int& bm, int& bn, int& ks) {
    ks = code >= VARIANT_FLAG ? code / VARIANT_FLAG : 1;
    bm = code % VARIANT_FLAG / 1000;
    bn = code % 1000;
}
inline int wgrad_variant_encode(int bmw, int bnw, bool norm) { return bmw * 1000 + bnw + (norm ? VARIANT_FLAG : 0); }
inline void wgrad_variant_decode(int code, int& bmw, int& bnw, bool& norm) {
    norm = code >= VARIANT_FLAG;
    bmw = code % VARIANT_FLAG / 1000;
    bnw = code % 1000;
}

}  // namespace fn
