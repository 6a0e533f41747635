/* C ABI of libfacenet_hip.so -- the MI355X (gfx950) drop-in boundary for the
 * sMedX/FaceNet training/inference hot path.
 *
 * The reference has no FFI of its own: its hot path is the set of TensorFlow /
 * Keras ops called from facenet/models/inception_resnet_v1.py, facenet/facenet.py,
 * facenet/statistics.py and apps/train_softmax.py.  Every entry point below
 * cites the reference call site(s) whose arithmetic it replaces.
 *
 * Conventions: plain pointers and sizes only; every pointer is DEVICE memory
 * owned by the caller (activations NHWC, low precision = bf16 or f16 selected
 * by `dtype`; parameters/gradients fp32); kernels never allocate; every call
 * is asynchronous on `stream` (a hipStream_t) and is HIP-graph capturable;
 * return 0 on success, negative on error with text in fn_last_error()
 * (thread-local).  No global mutable state: calls are re-entrant.
 */
#ifndef FACENET_HIP_H
#define FACENET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FN_BF16 0
#define FN_F16 1

/* Order-independent accumulators.  Sums that many workgroups contribute to -- BatchNorm batch statistics, the BatchNorm-backward
 * sums, bias gradients, the losses -- are 64-bit FIXED-POINT integers: every workgroup converts its fp32 partial sum once (round
 * to nearest) and adds it with an integer atomic, so the total has the same bits whatever order the workgroups arrive in and a
 * training step is reproducible bit for bit (fp32 atomics were not).  value = integer * 2^-bits.  Forward statistics use
 * FN_ACC_STAT_BITS (|sum| < 8.8e12), gradient sums FN_ACC_GRAD_BITS (|sum| < 8.4e6, resolution 9e-13).  Callers zero them
 * (all-zero bits) and read them back with fn_acc_to_float or by scaling on the host. */
typedef int64_t fn_acc_t;
#define FN_ACC_STAT_BITS 20
#define FN_ACC_GRAD_BITS 40

const char* fn_last_error(void);
int fn_abi_version(void);

/* ---- convolution as implicit GEMM on MFMA ------------------------------------
 * Replaces tf.keras.layers.Conv2D (+ the BatchNormalization statistics pass, ReLU,
 * bias, tf.concat and the residual "net += scale * up" that surround it):
 * inception_resnet_v1.py:90-138,160-193,215-248,269-299,316-367,387-430 (Conv2D),
 * :141-148,196-202,251-257 (concat + residual), :304-306,372-375 (concat),
 * and the Dense layers at :462 and apps/train_softmax.py:57-63 (a 1x1 conv on [N,1,1,C]).
 * The descriptor always states the FORWARD geometry of the layer. */
typedef struct fn_conv_desc {
    int32_t N, H, W, Cin;      /* forward input  [N,H,W,Cin]  */
    int32_t OH, OW, Cout;      /* forward output [N,OH,OW,Cout] */
    int32_t KH, KW, stride, pad_h, pad_w;
    int32_t dtype;             /* FN_BF16 | FN_F16 : activation + packed-weight storage */
    int32_t ld_x, ld_y;        /* channel stride (elements) of the x-side and y-side buffers (concat-free slices) */
    int32_t relu;              /* fwd epilogue: max(.,0) */
    int32_t accumulate;        /* fwd/dgrad epilogue: add to what `y`/`dx` already holds */
    int32_t out_f32;           /* fwd: y (dgrad: dx) is fp32 instead of low precision */
    int32_t ld_res;            /* channel stride of resid */
    float scale;               /* fwd: y = resid + scale*(conv + bias) when resid != NULL, else conv + bias */
    int32_t splits;            /* wgrad: split-K factor over pixels (0 = library picks) */
    int32_t stats_sq_off;      /* fwd: element offset from the sum array to the sum-of-squares array in `stats` */
    int32_t stats_replicas;    /* fwd: number of accumulator replicas (row tile t adds into replica t % replicas); 0/1 = one */
    int32_t stats_rep_stride;  /* fwd: element stride between replicas */
    const void* x;             /* fwd/wgrad: input activations; dgrad: unused */
    const void* w;             /* fwd: packed [Cout][KH*KW*Cin]; dgrad: transposed pack [Cin][KH*KW*Cout] */
    void* y;                   /* fwd: output; dgrad/wgrad: dY (read) */
    void* dx;                  /* dgrad: output dX [N,H,W,ld_x] */
    float* dw;                 /* wgrad: fp32 [Cout][KH*KW*Cin], atomically accumulated (caller zeroes) */
    const float* bias;         /* fwd: per-Cout fp32 or NULL (BN-folded shift / `up` bias) */
    fn_acc_t* stats;           /* fwd: NULL or fixed point (FN_ACC_STAT_BITS): stats[c] += sum, stats[stats_sq_off + c] += sum of squares (BN batch statistics) */
    const void* resid;         /* fwd: residual trunk [N,OH,OW,ld_res] or NULL */
    /* dgrad: optional fused reduction of the BatchNorm backward of the layer that produced x (see fn_bn_relu_train_bwd):
     * bn_y = that layer's raw output (same slice as dx), bn_acc[rep*stride + c] += sum dyh, [.. + bn_sq_off + c] += sum dyh*xhat */
    const void* bn_y;
    const float* bn_scale;
    const float* bn_shift;
    const float* bn_beta;
    fn_acc_t* bn_acc;          /* fixed point, FN_ACC_GRAD_BITS */
    int32_t ld_bn_y, bn_sq_off, bn_replicas, bn_rep_stride, bn_relu;
    /* fwd / wgrad: "normalise on load".  When nrm_stats is set, x is the RAW output of a BatchNormalization(center only)+ReLU
     * layer whose batch statistics (sum | sum of squares, replicated like `stats`) have been accumulated by the producing
     * fn_conv2d_fwd; the operand the convolution sees is relu((x - mean) * rstd + beta), computed per element while the tile
     * is staged (zero padding stays zero).  The activated tensor is then never written.  Index 0 of nrm_stats / nrm_beta
     * is channel 0 of x; nrm_count = N*H*W of x.  Cin <= 512.  fn_bn_finalize publishes the same scale / shift for the
     * backward pass and updates the moving statistics. */
    const fn_acc_t* nrm_stats; /* as `stats` */
    const float* nrm_beta;
    int32_t nrm_sq_off, nrm_replicas, nrm_rep_stride, nrm_count;
    float nrm_eps;
    /* fwd, optional with nrm_stats: the convolution also MATERIALISES the activated tensor it normalises -- nrm_z has the
     * geometry of x (same ld_x); every element is written exactly once, by the workgroups of the first Cout tile while they
     * stage the centre tap.  Needs stride 1 and OH x OW == H x W (1x1, or 'same' padding).  This replaces the
     * fn_bn_relu_train_fwd launch of the producing layer; the weight gradient then reads nrm_z like any activation. */
    void* nrm_z;
    /* fwd / dgrad tile variant: 0 = library heuristic, BM*1000+BN with BM, BN in {128, 64, 32} = caller's choice (the host side
     * times the candidates once per plan: facenet_amd/engine.py autotune), 9000000 = the halo-tile kernel (3x3, stride 1,
     * channels a multiple of 8; FN_EUNSUPPORTED otherwise) also where the heuristic would not pick it.  Results do not depend
     * on the tile beyond the summation order. */
    int32_t tile_fwd, tile_dgrad;
    /* dgrad of SIBLING 1x1 stride-1 layers that read the same x (inception towers branching off one trunk): dX = y-gradient of
     * this layer times its transposed pack PLUS the same for up to two more layers (dy2/w2, dy3/w3; their Cout and dy row
     * stride), computed as one GEMM whose K runs through the sources -- one launch and one pass over dX instead of a chain of
     * read-modify-write accumulations.  dy2 == NULL: ordinary single layer. */
    const void* dy2;
    const void* w2;
    const void* dy3;
    const void* w3;
    int32_t Cout2, ld_y2, Cout3, ld_y3;
    /* dgrad, optional: the RESIDUAL BACKWARD of the block whose output is x, fused into this launch's epilogue (it is the last
     * producer of that output's gradient; inception_resnet_v1.py:145-148,199-202,254-257: out = act(trunk + scale*(up + bias))).
     *   total = this data gradient + rb_prev        rb_prev : gradient x has received so far (geometry of dx), or NULL
     *   g     = rb_out ? total * (rb_out > 0) : total rb_out  : the block's forward output (ReLU mask), NULL = no activation
     *   rb_dtrunk (+)= g                             gradient of the block's trunk input; rb_accumulate: add to what it holds
     *   rb_dup = rb_scale * g                        gradient of the block's `up` convolution output
     *   rb_dbias[c] += sum over pixels of rb_dup     (fp32, the `up` bias gradient)
     * All four tensors have dx's geometry (ld_x).  dx itself is not written.  rb_dup == NULL: ordinary data gradient. */
    const void* rb_prev;
    const void* rb_out;
    void* rb_dtrunk;
    void* rb_dup;
    fn_acc_t* rb_dbias;        /* fixed point, FN_ACC_GRAD_BITS (fn_acc_to_float moves the bias gradients into the fp32 gradient buffer) */
    float rb_scale;
    int32_t rb_accumulate;
    /* fwd, optional: PReLU with one slope per output channel (Keras PReLU(shared_axes=[1,2]) after Conv2D, PReLU() after Dense:
     * the P/R/O-Net layers of the MTCNN detector behind detectors/face_detector.py:63-78): y = v > 0 ? v : prelu[c] * v,
     * applied to conv + bias.  Not combined with resid / relu / accumulate. */
    const float* prelu;
} fn_conv_desc;

/* One Inception-ResNet-B block ("Block17", inception_resnet_v1.py:153-204) of the BN-FOLDED inference network in ONE launch:
 * 1x1 | 1x1 -> 1x7 -> 7x1 towers, concat, `up` 1x1 + bias, scaled residual add, ReLU.  One workgroup per image; the tower
 * activations stay in LDS, only weights stream (csrc/block_fused.hip).  x, y: [N,8,8,896] low precision (x != y); weights: the
 * inference packs [Cout][taps][Cin] of the five layers (fn_fold_bn); b_t*: the folded BatchNorm shifts, b_up: the `up` bias.
 * Equals the five fn_conv2d_fwd launches it replaces up to the summation order. */
int fn_block17_infer(const void* x, void* y, int N, const void* w_t0, const void* w_t1a, const void* w_t1b, const void* w_t1c, const void* w_up,
                     const float* b_t0, const float* b_t1a, const float* b_t1b, const float* b_t1c, const float* b_up, float scale, int relu,
                     int dtype, void* stream);
/* fn_block17_infer plus 64 extra workgroups (on CUs the one-image-per-workgroup launch leaves idle) that read
 * [warm, warm + warm_bytes) into every XCD's L2: the bytes the NEXT launch streams, normally the next block's weight packs
 * (16-byte aligned, < 2 GiB).  Results are those of fn_block17_infer; warm == NULL (with warm_bytes 0) is fn_block17_infer. */
int fn_block17_infer_warm(const void* x, void* y, int N, const void* w_t0, const void* w_t1a, const void* w_t1b, const void* w_t1c,
                          const void* w_up, const float* b_t0, const float* b_t1a, const float* b_t1b, const float* b_t1c, const float* b_up,
                          float scale, int relu, const void* warm, int64_t warm_bytes, int dtype, void* stream);
/* One Inception-ResNet-A block ("Block35", inception_resnet_v1.py:83-150) of the BN-folded inference network in ONE launch (seven
 * convolution launches otherwise): x, y [N,17,17,256]; w_1x1 / b_1x1: the three tower-entry 1x1 layers (tower_conv0/Conv2d_1x1,
 * tower_conv1/Conv2d_0a_1x1, tower_conv2/Conv2d_0a_1x1); w_3x3 / b_3x3: tower_conv1/Conv2d_0b_3x3, tower_conv2/Conv2d_0b_3x3,
 * tower_conv2/Conv2d_0c_3x3; w_up / b_up: the `up` layer [256][96] and its bias.  Arrays of 3 device pointers (host arrays). */
int fn_block35_infer(const void* x, void* y, int N, const void* const* w_1x1, const void* const* w_3x3, const void* w_up,
                     const float* const* b_1x1, const float* const* b_3x3, const float* b_up, float scale, int relu, int dtype, void* stream);
/* fn_block35_infer plus the warm-ahead workgroups of fn_block17_infer_warm (same contract for warm / warm_bytes). */
int fn_block35_infer_warm(const void* x, void* y, int N, const void* const* w_1x1, const void* const* w_3x3, const void* w_up,
                          const float* const* b_1x1, const float* const* b_3x3, const float* b_up, float scale, int relu,
                          const void* warm, int64_t warm_bytes, int dtype, void* stream);
int fn_conv2d_fwd(const fn_conv_desc* d, void* stream);
int fn_conv2d_dgrad(const fn_conv_desc* d, void* stream);
int fn_conv2d_wgrad(const fn_conv_desc* d, void* stream);
/* Grouped forward / data-gradient convolutions: one launch for n INDEPENDENT layers that share a tile variant
 * (= fn_conv2d_variant(d, op)) and 1x1-ness (plain).  Planned on the host like the grouped weight gradients below. */
int fn_conv2d_arg_bytes(void);
int fn_conv2d_group_build(const fn_conv_desc* descs, int n, int op, int variant, void* host_args, int32_t* host_prefix, int32_t* smem_bytes);
int fn_conv2d_grouped(const void* dev_args, const int32_t* dev_prefix, int n, int total_blocks, int variant, int plain, int smem_bytes,
                      int dtype, void* stream);
/* Grouped weight gradients: one launch for many layers that share a tile variant (= fn_conv2d_variant(d, 2)).
 * fn_conv2d_wgrad_group_build plans on the HOST: it fills host_args (n * fn_conv2d_wgrad_arg_bytes() bytes, opaque) and
 * host_prefix (n+1 workgroup offsets) and returns the total workgroup count; the caller copies both to device memory once and
 * replays fn_conv2d_wgrad_grouped every step (pointers inside the descriptors must stay valid).  Members that normalise x
 * on load (nrm_stats) form groups of their own: pass variant + 1000000 to both calls.  Likewise fn_conv2d_grouped takes
 * plain | 2 for a group whose members all normalise on load. */
int fn_conv2d_wgrad_arg_bytes(void);
int fn_conv2d_wgrad_group_build(const fn_conv_desc* descs, int n, int variant, void* host_args, int32_t* host_prefix, float* ws,
                                int64_t* ws_elems);
int fn_conv2d_wgrad_grouped(const void* dev_args, const int32_t* dev_prefix, int n, int total_blocks, int variant, int dtype, void* stream);
/* The grouped path is deterministic and free of atomics: a layer that is not split over pixels stores dw directly; a split layer
 * stores split z into slab z of the workspace `ws` (fp32 [splits][Cout*K] per layer, laid out by group_build) and
 * fn_conv2d_wgrad_reduce, launched after fn_conv2d_wgrad_grouped with the same dev_args, writes dw = slab 0 + slab 1 + ... in that
 * order.  Call group_build once with ws = NULL to learn *ws_elems (floats), allocate, and call it again with the pointer.  dw
 * needs no zeroing on this path.  (fn_conv2d_wgrad, the single-layer launch, still accumulates atomically into a zeroed dw.) */
int fn_conv2d_wgrad_reduce(const void* dev_args, int n, void* stream);
/* tile variant the descriptor dispatches to (op 0 fwd, 1 dgrad, 2 wgrad): BM*1000+BN; measurement aid only */
int fn_conv2d_variant(const fn_conv_desc* d, int op);

/* ---- input normalisation: facenet/facenet.py:67-86 (ImageProcessing.call) -------
 * u8 NHWC [N,H,W,3] -> low precision [N,H,W,8] (channels 3..7 zero), mode 0 = per-image
 * min/max to [-1,1], mode 1 = per_image_standardization.  `work` = 8*N 32-bit words of scratch (8-byte aligned). */
int fn_image_normalize(const uint8_t* img, void* out, float* work, int N, int HW, int mode, int dtype, void* stream);
int fn_image_normalize_f32(const float* img, void* out, float* work, int N, int HW, int mode, int dtype, void* stream);
/* tf.image.resize(images, [size,size]) of facenet.py:70 (bilinear, half-pixel centres, no antialias): u8 or fp32 NHWC
 * [N,H,W,3] -> fp32 [N,OH,OW,3]; the identity at the configured size, so plans skip it then. */
int fn_image_resize_bilinear(const void* img, int src_is_f32, float* out, int N, int H, int W, int OH, int OW, void* stream);
/* tf.image.resize_with_crop_or_pad(image, size, size) of ImageLoader.__call__ (facenet.py:45-54) for a ragged batch of decoded
 * HWC u8 images packed back to back: image n starts at byte offsets[n] of src and is hw[2n] x hw[2n+1] x 3; centre crop
 * (offset max((h-S)//2, 0)) and centre zero-pad (offset max((S-h)//2, 0)) to dst u8 [N,S,S,3].  Sizes are not checked against
 * the src allocation: the caller owns the packing. */
int fn_crop_or_pad_u8(const uint8_t* src, const long long* offsets, const int32_t* hw, uint8_t* dst, int N, int S, void* stream);
/* Training-time augmentation (image.random_rotate / random_crop / random_flip), one record per image:
 *   y0, x0   signed offset of the S x S window in the rotated image R (R has the source's size h x w): C[y][x] = R[y+y0][x+x0]
 *            where that lies inside R, else 0.  >= 0 crops at that offset, < 0 zero-pads by -y0 / -x0.
 *   flip     non-zero: out[y][x] = C[y][S-1-x]
 *   cos_t, sin_t  of the rotation angle.  R[y][x] is the bilinear sample (zero outside the source) of the source at
 *            sx = c*u - s*v + w/2 - 0.5, sy = s*u + c*v + h/2 - 0.5 with u = x + 0.5 - w/2, v = y + 0.5 - h/2, in fp32 without
 *            contraction, rounded half-to-even and clamped to [0, 255].  (sin_t, cos_t) == (0, 1) is a pure byte copy. */
typedef struct fn_augment_param {
    int32_t y0, x0;
    int32_t flip;
    float cos_t, sin_t;
} fn_augment_param;
/* fn_crop_or_pad_u8's ragged src / offsets / hw input and one fn_augment_param per image (device memory) -> dst u8 [N,S,S,3] in
 * one launch; S must be even.  Sizes are not checked against the src allocation: the caller owns the packing. */
int fn_augment_u8(const uint8_t* src, const long long* offsets, const int32_t* hw, const fn_augment_param* params, uint8_t* dst, int N,
                  int S, void* stream);
/* A batch from a data set whose decoded pixels live in device memory: `pool`, `offsets` (byte offsets, 64-bit,
 * any alignment) and `hw` are the tables of the whole set of M images, and image n of the batch is row rows[n] of them, so no
 * per-batch table is gathered.  With `params` (one record per batch image) dst is what fn_augment_u8 writes for the same images and
 * records, byte for byte; with params == NULL every image gets the centre crop / pad of fn_crop_or_pad_u8, computed from hw.
 * A row outside [0, M) is defined: neither the tables nor the pool are read for it, its output image is all zero and the other
 * images of the batch are unaffected.  N <= 65535, S even.  Rows inside [0, M) are not checked against the pool allocation: the
 * caller owns the tables. */
int fn_resident_batch_u8(const uint8_t* pool, const long long* offsets, const int32_t* hw, long long M, const int32_t* rows,
                         const fn_augment_param* params, uint8_t* dst, int N, int S, void* stream);
/* PIL's `frame.crop(window).resize((side, side), LANCZOS)` for 8-bit RGB, bit for bit, for F windows over
 * one HWC u8 frame [H,W,3] in device memory.  `windows` is HOST memory, F x (left, top, right, bottom) with exclusive right /
 * bottom; a window may reach outside the frame on any side (those pixels of the crop are 0).  dst u8 [F,S,S,3] holds rows / columns
 * [oy, oy+S) x [ox, ox+S) of each side x side result: ox = oy = 0, S = side is the whole thumbnail, ox = oy = (side - size) / 2,
 * S = size the centre cut that fn_crop_or_pad_u8 would take from it.  Limits: side <= FN_FACE_CROP_MAX_SIDE, every window
 * 1 .. FN_FACE_CROP_MAX_EXTENT pixels per axis (the rows one output row needs must fit 64 KiB of LDS at any side), F <= 65535.
 * `workspace` is device memory of at least the int32 words fn_face_crop_workspace reports for the same windows and side; the
 * windows are copied into it on `stream`, then one table launch and one resampling launch follow. */
#define FN_FACE_CROP_MAX_SIDE 256
#define FN_FACE_CROP_MAX_EXTENT 3072
int fn_face_crop_workspace(const int32_t* windows, int F, int side, long long* words);
int fn_face_crop_resize_u8(const uint8_t* frame, int H, int W, const int32_t* windows, int F, int side, int ox, int oy, int S, uint8_t* dst,
                           int32_t* workspace, long long workspace_words, void* stream);
/* Landmark alignment: F faces of one HWC u8 frame [H,W,3] in device memory, each warped through its own
 * inverse similarity transform onto dst u8 [F,S,S,3].  `inverse` is HOST memory, F x (i0, i1, i2, i3, i4, i5): sub-sample
 * (uu, vv) of the output reads the frame at x = (i0 uu + i1 vv) + i2, y = (i3 uu + i4 vv) + i5 with bilinear taps that are 0
 * outside the frame; `samples` is HOST memory, F x n: output pixel (u, v) is the mean, rounded half to even, of its n x n
 * sub-samples uu = u + ((i + 0.5) / n - 0.5), likewise vv (a box prefilter; n = 1 is the plain bilinear warp).  All fp64 without
 * contraction.  Limits: F <= 65535, S <= FN_FACE_ALIGN_MAX_SIDE, 1 <= n <= FN_FACE_ALIGN_MAX_SAMPLES, every inverse entry
 * finite and below 2^24 in magnitude.  `workspace` is 8-byte aligned device memory of at least the bytes
 * fn_face_align_workspace reports; both tables are copied into it on `stream`, then one launch follows. */
#define FN_FACE_ALIGN_MAX_SIDE 256
#define FN_FACE_ALIGN_MAX_SAMPLES 8
int fn_face_align_workspace(int F, long long* bytes);
int fn_face_align_u8(const uint8_t* frame, int H, int W, const double* inverse, const int32_t* samples, int F, int S, uint8_t* dst,
                     void* workspace, long long workspace_bytes, void* stream);
/* gather rows of a u8 image pool by index (triplet batch assembly): out[i] = pool[idx[i]].  bytes_per_image must be a multiple
 * of 16 (the images are copied as 16-byte vectors; fn_crop_or_pad_u8 / fn_augment_u8 refuse odd sizes likewise, so a 299 x 299 x 3
 * pool is not supported); anything else is rejected before the launch. */
int fn_gather_images(const uint8_t* pool, const int32_t* idx, uint8_t* out, int n_out, int bytes_per_image, void* stream);

/* Batched finalisation for the layers consumed through nrm_* (no fn_bn_relu_train_fwd launch): for every channel c < CB with
 * reps[c] > 0: mean/var from the replicated sums (count[c] elements), save_scale = rstd, save_shift = beta - mean*rstd,
 * moving statistics updated as in fn_bn_relu_train_fwd.  One launch for the whole network. */
int fn_bn_finalize(const fn_acc_t* stats, int sq_off, int rep_stride, const int32_t* reps, const int32_t* count, const float* beta,
                   float* save_scale, float* save_shift, float* moving_mean, float* moving_var, float momentum, float eps, int CB,
                   void* stream);

/* ---- BatchNormalization (center only, no scale; eps 1e-3, momentum 0.99) --------
 * inception_resnet_v1.py:56-63 and every BatchNormalization(**...) line; ReLU() fused.
 * Training: y (raw conv output, channel slice [0,C) of a [M,ld_y] buffer) -> z = relu((y-mean)*rstd+beta)
 * with batch statistics from `stats` (sum,sumsq as written by fn_conv2d_fwd); scale=rstd and
 * shift=beta-mean*rstd are saved for backward and the moving statistics are updated (biased variance). */
int fn_bn_relu_train_fwd(const void* y, int ld_y, void* z, int ld_z, int M, int C, const fn_acc_t* stats, int stats_sq_off, int stats_replicas,
                         int stats_rep_stride, const float* beta,
                         float* save_scale, float* save_shift, float* moving_mean, float* moving_var, float momentum, float eps,
                         int relu, int dtype, void* stream);
/* backward: dz (grad wrt the BN+ReLU output) -> dy (grad wrt the raw conv output y), in place; y is the raw forward
 * conv output (xhat and the ReLU mask are recomputed from it: masked elements still receive the batch-statistic
 * terms).  acc (zeroed by the caller) holds sum dyh at acc[rep*stride + c] and sum dyh*xhat at acc[rep*stride + acc_sq_off + c];
 * with reduced = 0 this call fills it (reduce kernel, replica 0), with reduced = 1 a fn_conv2d_dgrad epilogue already did.
 * dbeta[C] += sum dyh. */
int fn_bn_relu_train_bwd(void* dz, int ld_d, const void* y, int ld_y, int M, int C, const float* beta, const float* save_scale,
                         const float* save_shift, float* dbeta, fn_acc_t* acc, int acc_sq_off, int acc_replicas, int acc_rep_stride,
                         int reduced, int relu, int dtype, void* stream);

/* ---- pooling: MaxPool2D(3, strides=2, 'valid') :301,369,409 ; AvgPool2D([3,3]) + Flatten :460-461 */
/* argmax (optional, u8 [N,OH,OW,C]): scan position 0..8 of the FIRST maximum of every window; when given to the backward it
 * replaces the recomputation from x (x may then be NULL).
 * Precondition: every window holds a value > -3.0e38 (the running maximum starts there): a window made only of -Inf, or of
 * finite values below -3.0e38 (bf16 can hold them), yields -3.0e38 rounded to the storage type and argmax 0.  The network
 * pools post-ReLU maps; ordinary negative values are handled exactly.  H == 4 / W == 4 and other sizes where (H - 3) is odd
 * leave the last row / column outside every window: the backward writes 0 there (or keeps the value under accumulate). */
int fn_maxpool3x3s2_fwd(const void* x, int ld_x, void* y, int ld_y, int N, int H, int W, int C, uint8_t* argmax, int dtype, void* stream);
int fn_maxpool3x3s2_bwd(const void* x, int ld_x, const void* dy, int ld_dy, void* dx, int ld_dx, int N, int H, int W, int C,
                        const uint8_t* argmax, int accumulate, int dtype, void* stream);
/* ---- MTCNN face detector (detectors/face_detector.py:63-78 wraps PyPI `mtcnn`; apps/extract_faces.py:30,56) -------------
 * The P/R/O-Net convolutions and dense layers are fn_conv2d_fwd launches (bias + fn_conv_desc.prelu); these three entry points
 * are the rest of the device work.  Arithmetic restated in oracle/mtcnn_oracle.py (parity unpinned: the package and cv2 are
 * not installed).
 * fn_area_resize_crop: for k < n, boxes[4k..] = (ox, oy, cw, ch) is a crop of the uint8 HWC frame (zero outside the frame),
 *   resized to OH x OW like cv2.resize(crop, (OW, OH), interpolation=cv2.INTER_AREA) -- true area resampling when both axes
 *   shrink, cv2's area-mode bilinear otherwise -- then (v - 127.5) * 0.0078125 and stored TRANSPOSED as out[k][x][y][8] low
 *   precision (channels 3..7 zero): the networks were trained on transposed images.  source_is_u8 = 1: the crop is a uint8
 *   image (float accumulators, result rounded half-to-even to uint8: the stage-1 pyramid); 0: the crop is float64 (stages 2, 3:
 *   double accumulators, no rounding; the enlarging path is only built for this case). */
int fn_area_resize_crop(const uint8_t* frame, int H, int W, const int32_t* boxes, int n, int OH, int OW, int source_is_u8, void* out,
                        int dtype, void* stream);
/* MaxPooling2D(pool_size=k, strides=stride, 'valid' or 'same'): pad_h / pad_w = Keras' padding BEFORE (0 for every MTCNN
 * layer), windows are clipped at the border, OH / OW as Keras computes them. */
int fn_maxpool2d_fwd(const void* x, int ld_x, void* y, int ld_y, int N, int H, int W, int C, int k, int stride, int pad_h, int pad_w,
                     int OH, int OW, int dtype, void* stream);
/* Whole-frame pyramid level (source_is_u8 case of fn_area_resize_crop with the window = the frame, same results bit for bit) in
 * two passes, horizontal then vertical -- the order cv2 itself works in; rows: fp32 workspace [H][OW][3].  OH <= H, OW <= W. */
int fn_area_resize_frame(const uint8_t* frame, int H, int W, int OH, int OW, float* rows, void* out, int dtype, void* stream);
/* P-Net map [ncell][ld] fp32 = (logit0, logit1, reg0..3, ...) per cell: p1 = softmax(logits)[1]; cells with p1 >= threshold are
 * appended to cand (16-byte aligned) as 8-float records (cell index as int bits, tag as int bits, p1, reg0..3, 0) in any order;
 * `tag` lets the levels of a pyramid share one buffer.  *counter += number of hits (may exceed max_cand: only records below
 * max_cand are stored); reset_counter: zero it first. */
int fn_mtcnn_candidates(const float* map, long ncell, int ld, float threshold, float* cand, int32_t* counter, int max_cand, int tag,
                        int reset_counter, void* stream);
/* Greedy NMS of the package (__nms): boxes [n][ld] float64 rows (x1, y1, x2, y2, ...), order = np.argsort(scores) (ascending; the
 * best box is order[n-1]), ratio = inter / (area_i + area_j - inter) or, by_min, inter / min(area_i, area_j), all in float64 with
 * the package's operation order; a box survives while every better kept box has ratio <= threshold.  keep[0..*n_keep) = indices
 * of the kept boxes, best first.  workspace: n * ceil(n / 64) * 8 bytes (pairwise bit matrix).
 * _batch: njobs independent jobs in one pair of launches (one workgroup scans each job); boxes / order / keep are concatenated in
 * job order, sizes / thresholds / by_min are HOST arrays of njobs entries, n_keep[j] per job, workspace = sum of the jobs'. */
int fn_nms_greedy(const double* boxes, int ld, const int32_t* order, int n, double threshold, int by_min, void* workspace,
                  long workspace_bytes, int32_t* keep, int32_t* n_keep, void* stream);
int fn_nms_greedy_batch(const double* boxes, int ld, const int32_t* order, const int32_t* sizes, const double* thresholds, const int32_t* by_min,
                        int njobs, void* workspace, long workspace_bytes, int32_t* keep, int32_t* n_keep, void* stream);
int fn_avgpool_fwd(const void* x, void* y, int N, int HW, int C, int dtype, void* stream);
int fn_avgpool_bwd(const void* dy, void* dx, int N, int HW, int C, int dtype, void* stream);
/* Inception-ResNet-v2: AvgPool 3x3 / stride 1 / SAME over an NHWC channel slice (ld = channel stride of the buffer); the divisor is
 * the number of in-map taps (TF).  bwd: dx (+)= the gather of dy/taps over the covering windows (accumulate = 1 adds). */
int fn_avgpool3x3s1_fwd(const void* x, int ld_x, void* y, int ld_y, int N, int H, int W, int C, int dtype, void* stream);
int fn_avgpool3x3s1_bwd(const void* dy, int ld_dy, void* dx, int ld_dx, int N, int H, int W, int C, int accumulate, int dtype,
                        void* stream);
/* Dropout on [N,C] (C % 8 == 0, 0 < keep < 1): y = x/keep where lowbias32-fold(seed, rank, *step, n, c) < round(keep * 2^32), else 0.
 * step is a device int32 read by the kernel (HIP-graph replays see it advance); bwd applies the same mask to dy. */
int fn_dropout_fwd(const void* x, void* y, int N, int C, float keep, unsigned seed, int rank, const int32_t* step, int dtype, void* stream);
int fn_dropout_bwd(const void* dy, void* dx, int N, int C, float keep, unsigned seed, int rank, const int32_t* step, int dtype, void* stream);

/* ---- residual backward for "net = act(net + scale*up)" (:145-148,199-202,254-257) ------------
 * dpre = dout * (out>0 if relu); dtrunk = dpre (or += when accumulate); dup = scale*dpre; dbias[C] += sum(dup). */
int fn_residual_bwd(const void* dout, const void* out, void* dtrunk, void* dup, fn_acc_t* dbias, int M, int C, float scale, int relu,
                    int accumulate, int dtype, void* stream);

/* dst[i] = src[i] * 2^-bits (the bias gradients leave their fixed-point accumulators for the fp32 gradient buffer) */
int fn_acc_to_float(const fn_acc_t* src, float* dst, long n, int bits, void* stream);

/* ---- embedding head on fp32 [N,E]: BN without ReLU (:467) and tf.nn.l2_normalize (:491-492) ---- */
int fn_head_bn_fwd(const float* y, float* out, int N, int E, const float* beta, float* moving_mean, float* moving_var,
                   float* save_mean, float* save_rstd, int training, float momentum, float eps, void* stream);
int fn_head_bn_bwd(const float* dout, const float* y, const float* save_mean, const float* save_rstd, float* dbeta, void* dy_lp,
                   int N, int E, int dtype, void* stream);
int fn_l2norm_fwd(const float* x, float* out, int N, int E, float eps, void* stream);
int fn_l2norm_bwd(const float* x, const float* dout, float* dx, int N, int E, float eps, void* stream);
int fn_cast_f32_to_lp(const float* x, void* y, long n, int dtype, void* stream);

/* ---- distances / triplets ---------------------------------------------------------------------
 * fn_pairwise_sqdist: facenet/statistics.py:22-57 (pairwise_similarities): metric 0 -> 2(1-a.b) with the
 * dot clipped to [-1,1], metric 1 -> arccos, metric 2 -> |a|^2+|b|^2-2a.b (un-normalised inputs).
 * range[2] receives min/max of the raw dot products (the reference's +-(1+atol) check is done by the caller).
 * Triplet selection / loss are build-defined (arXiv 1503.03832 sec. 3). */
int fn_pairwise_sqdist(const float* xa, const float* xb, float* out, float* range, int n, int m, int E, int metric, void* stream);
/* fn_select_triplets: labels must hold at least two different values.  A pair whose anchor has no row of another label has no
 * negative; its triplet slot is left unwritten.  facenet_amd.triplet.select_triplets and TripletMiner reject such pools on the
 * host.  info (int32 [8 + 5 n(n-1)/2], zeroed once by the caller): [0] pairs, [1] pairs with a candidate, [2] 1 if fewer pairs
 * than nrof_triplets, [3] call counter (the effective seed is seed + info[3]). */
int fn_select_triplets(const float* dist, const int32_t* labels, int n, float alpha, int nrof_triplets, uint32_t seed,
                       int semi_hard, int32_t* triplets, int32_t* info, void* stream);
/* loss: fp32[4] -- word 0 receives the loss; words 2-3 are the launch's own fixed-point accumulator (FN_ACC_GRAD_BITS) */
int fn_triplet_loss_fwd_bwd(const float* emb, float* demb, float* loss, int T, int E, float alpha, void* stream);
/* Batch-mined triplet losses on a whole batch (arXiv 1703.07737 sec. 2).
 * emb fp32 [N,E] (unit norm is not assumed); dist fp32 [N,N] = fn_pairwise_sqdist(emb, emb, metric 2), bitwise symmetric; labels
 * int32 [N], any values; 2 <= N <= 1024, 1 <= E <= 512.  strategy 0 = batch hard (per anchor the farthest positive and the nearest
 * negative, the lowest index on ties), 1 = batch all (every valid triplet).  soft 0 = hinge max(d_ap - d_an + alpha, 0), active
 * iff strictly > 0 (alpha finite, >= 0); soft 1 = softplus(d_ap - d_an), alpha ignored.
 * info int32 [8]: [0] anchors with a positive and a negative, [1] terms, [2] active terms (soft: = [1]), [3] 1 if a distance of
 * such an anchor to one of its positives or negatives was not finite (loss[0] is then NaN), [4..7] zero.
 * Z = info[0] (batch hard), info[2] (batch all, hinge), info[1] (batch all, soft); Z = 0 gives loss 0 and a zero gradient.
 * coef fp32 [N,N], written in full: coef[a][j] = d (Z loss) / d dist[a][j] with a as the anchor (> 0 for a positive j, < 0 for a
 * negative j, else 0).  demb fp32 [N,E] or NULL: demb[r] = (2/Z) sum_j (coef[r][j] + coef[j][r]) (emb[r] - emb[j]), j ascending;
 * every row is written.  loss: fp32[4], 8-byte aligned, word 0 receives the loss.  No float atomics: bitwise reproducible. */
int fn_batch_triplet_fwd_bwd(const float* emb, const float* dist, const int32_t* labels, float* demb, float* loss, float* coef,
                             int32_t* info, int N, int E, float alpha, int strategy, int soft, void* stream);
/* Batch hard over the batch and a cross-batch memory (Wang et al., CVPR 2020).  emb, dist, labels, demb, loss,
 * coef, alpha, soft: as fn_batch_triplet_fwd_bwd with strategy 0; labels must name the same identity in every step.
 * mem_emb fp32 [M,E], mem_labels int32 [M], mem_state int32 [4] = cursor | valid rows | enqueue calls seen | 0: the ring that
 * fn_xbm_enqueue fills; mem_dist fp32 [N,M] = fn_pairwise_sqdist(emb, mem_emb, metric 2).  N <= M <= 65536.
 * The candidates of anchor a are the batch columns j != a (union index j) and the slots s < mem_state[1], read on the device (union
 * index N + s); slots at or beyond it are never looked at.  A row with a positive and a negative in the union is an anchor and gives
 * one term from its farthest positive and nearest negative, compared as fp32, the lowest union index on ties.
 * coef [N,N]: the picks that are batch columns.  mpick int32 [N,2]: the memory slot of the positive and of the negative pick, -1
 * where the pick is a batch column or the row is no anchor.  mcoef fp32 [N,2]: +c and -c for those slots (c = 1, sigma(l), or 0
 * for an inactive hinge).  info int32 [8]: [0..3] as fn_batch_triplet_fwd_bwd ([3] also covers the valid slots), [4] anchors whose
 * positive is a memory slot, [5] whose negative is, [6] the valid rows seen, [7] zero.  loss = sum / info[0].
 * demb [N,E] or NULL: (2/Z) times the chain of fn_batch_triplet_fwd_bwd followed by mcoef[r][0] (emb[r] - mem_emb[mpick[r][0]]) and
 * mcoef[r][1] (emb[r] - mem_emb[mpick[r][1]]).  The memory receives no gradient.  No float atomics: bitwise reproducible. */
int fn_xbm_triplet_fwd_bwd(const float* emb, const float* dist, const int32_t* labels, const float* mem_emb, const float* mem_dist,
                           const int32_t* mem_labels, const int32_t* mem_state, float* demb, float* loss, float* coef, int32_t* mpick,
                           float* mcoef, int32_t* info, int N, int M, int E, float alpha, int soft, void* stream);
/* One step of the ring, entirely on the device (a replayed graph advances it): while mem_state[2] < start the call is only counted;
 * afterwards row i of emb [N,E] and labels [N] goes to slot (cursor + i) mod M, then cursor <- (cursor + N) mod M, valid <-
 * min(valid + N, M).  mem_state[2] counts every call and saturates.  1 <= N <= min(M, 1024), M <= 65536, 1 <= E <= 512, start >= 0. */
int fn_xbm_enqueue(const float* emb, const int32_t* labels, float* mem_emb, int32_t* mem_labels, int32_t* mem_state, int N, int M,
                   int E, int start, void* stream);

/* ---- face-to-face validation statistics: facenet/statistics.py:111-138 (ConfidenceMatrix) with the class-balanced
 * weights of SimilarityCalculator.evaluate (:92-103).  emb fp32 [n,E], unit-norm rows grouped by class (class c = rows
 * cls_start[c] .. cls_start[c+1]); thresholds ascending, T <= 256; out fp64 [4*T] = tp | tn | fp | fn;
 * range[2] = ordered-int min/max of the raw dot products (for the reference's +-(1+atol) check, :40-42). */
int fn_confidence_counts(const float* emb, const int32_t* cls_start, int C, int E, const float* thresholds, int T, int metric,
                         double* out, int32_t* range, void* stream);

/* The tables of all F training parts of a k-fold validation in one pass over the pairs.  fold int32 [n]: the fold a row
 * is held out in (0 <= fold < F, 2 <= F <= 16); train_rows int32 [C*F]: rows of class c that are NOT held out in fold f;
 * train_classes int32 [F]: classes with at least one such row.  out fp64 [F*4*T]: out[f] is what fn_confidence_counts
 * gives for the rows with fold != f (classes without such a row removed); range covers the pairs that belong to at
 * least one training part.  Dot products are the same fp32 fmaf chains as fn_confidence_counts (exact fp32 MFMA). */
int fn_confidence_counts_folds(const float* emb, const int32_t* cls_start, const int32_t* fold, const int32_t* train_rows,
                               const int32_t* train_classes, int C, int E, int F, const float* thresholds, int T, int metric,
                               double* out, int32_t* range, void* stream);

/* ---- the exact verification curve: windowed histograms of the keys of ALL pairs, per population.  emb,
 * cls_start, C, metric and range: as fn_confidence_counts; E a multiple of 4 in [4, 512]; emb and out 16-byte aligned.  A pair of
 * rows of one class is genuine (population 0), any other pair an impostor (population 1); every unordered pair of distinct rows is
 * evaluated once.  Its key k is the bit pattern of its fp32 distance d (d >= +0, so keys order as distances do), d the very bits
 * of fn_confidence_counts, fn_gallery_search and fn_radius_*.  lo uint32 [R], shift int32 [R]: HOST arrays,
 * 1 <= R <= 8 windows of 1024 bins, 0 <= shift <= 22; a pair lands in bin (k - lo[r]) >> shift[r] of window r when k >= lo[r] and
 * that bin is < 1024.  out uint64 [R][2][1024 + 2], zeroed by the caller: per window and population the 1024 bins, the number of
 * pairs with k < lo[r], the population's number of pairs.  Counts are added with 64-bit integer atomics: the result does not
 * depend on scheduling.  The call allocates nothing and does not synchronise. */
int fn_pair_key_histogram(const float* emb, const int32_t* cls_start, int C, int E, int metric, const uint32_t* lo,
                          const int32_t* shift, int R, unsigned long long* out, int32_t* range, void* stream);

/* ---- false examples: the worst pairs at a threshold, picked greedily as facenet/statistics.py:334-421 does.
 * emb, cls_start, C, E, metric and range: as fn_pair_key_histogram; d is the same distance, bit for bit; no class may have more
 * than 65536 rows (the tie-break position is two 16-bit row numbers; the caller checks it).  False negatives, per class: the pair
 * (i < k) of not yet excluded rows with the largest d, ties to the smallest i, then k; emitted when d > threshold (strict fp32),
 * and both rows are excluded from the class's further picks; at most max_fneg picks.  False positives, per pair of classes a < b:
 * the pair (i in a, k in b) with row i and column k not yet excluded and the smallest d, ties to the smallest i, then k; emitted
 * when d < threshold, and row i and column k are excluded; at most max_fpos picks.  0 <= max_fneg, max_fpos <= 64.
 * count uint64 [2], zeroed by the caller: [0] the false negatives, [1] the false positives found, whatever the capacity.
 * records int32 [capacity][4], 16-byte aligned (NULL with capacity 0): {row1, row2, bits of d, pick index within its class (pair)},
 * rows of the sorted table, row1 < row2 (the lower class's row first).  False negative number s (in arrival order, which is not
 * deterministic) is records[s], false positive number s is records[capacity - 1 - s]; one beyond the capacity is counted and not
 * written, so the records are complete exactly when count[0] + count[1] <= capacity.  The call allocates nothing and does not
 * synchronise. */
int fn_false_pairs(const float* emb, const int32_t* cls_start, int C, int E, int metric, float threshold, int max_fneg, int max_fpos,
                   int32_t* records, long long capacity, unsigned long long* count, int32_t* range, void* stream);

/* ---- 1:N identification: for each of Q query rows the k nearest of G gallery rows; the [Q, G] distance
 * matrix never reaches memory.  s(q, g) is the same fp32 fmaf chain as fn_confidence_counts (exact fp32 MFMA), sc = s clipped to
 * [-1, 1]; rows are ranked by ascending (2 (1 - sc), gallery row) for both metrics, equal distances going to the lower row; dist
 * is 2 (1 - sc) (metric 0) or acosf(sc) (metric 1).  queries fp32 [Q, E], gallery fp32 [G, E], unit-norm rows, both and the
 * workspace 16-byte aligned; 1 <= k <= 64; E a multiple of 4 in [4, 512].  skip int32 [Q] or NULL: the gallery row query q must
 * not return (-1: none).  labels int32 [G] or NULL.  slab_rows: gallery rows per workgroup, rounded up to a multiple of 64 (0:
 * chosen by the library); the result does not depend on it.  workspace: at least the bytes fn_gallery_search_workspace reports
 * for the same Q, G, k and slab_rows.  dist fp32 [Q, k], rows int32 [Q, k], row_labels int32 [Q, k] or NULL (needs labels):
 * ascending; a query with fewer than k admissible rows gets row -1, dist +inf, label -1 in the tail.  range (2 words or NULL):
 * ordered-int min/max of s over all Q x G pairs, as in fn_pairwise_sqdist.  The caller owns every buffer; the call allocates
 * nothing and does not synchronise. */
int fn_gallery_search_workspace(int Q, int G, int k, int slab_rows, long long* bytes);
int fn_gallery_search(const float* queries, int Q, const float* gallery, int G, int E, int k, int metric, const int32_t* skip,
                      const int32_t* labels, int slab_rows, void* workspace, float* dist, int32_t* rows, int32_t* row_labels,
                      float* range, void* stream);

/* ---- the inverted-file index ------------------------------------------------------------------------------
 * fn_kmeans_update: the centroid step of spherical k-means.  rows fp32 [N, E] (E a multiple of 4 in [4, 512]); order int32 [N]: the
 * row numbers sorted by (list, row), both ascending; list_start int32 [L + 1]: list c's members are order[list_start[c] ..
 * list_start[c + 1]); prev fp32 [L, E]: the previous centroids.  sum[c][e] is the sequential fp64 sum, from 0.0, of (double)
 * rows[m][e] over the members m of c in ascending row order; n2[c] is the sequential fp64 sum, from 0.0 and over ascending e, of
 * the products sum[c][e] * sum[c][e], each rounded to fp64 before it is added (no fused multiply-add); centroids[c][e] =
 * (float)(sum[c][e] / sqrt(n2[c])), IEEE fp64 square root and division, one rounding to fp32.  A list without a member, or with
 * n2 == 0, keeps prev[c] bit for bit and gets kept[c] = 1; every other list kept[c] = 0.  centroids fp32 [L, E] must not be
 * prev; kept int32 [L].  No atomics: a call is reproducible bit for bit.
 *
 * fn_ivf_search: fn_gallery_search over the lists each query probes.  lists fp32 [G, E]: the gallery rows stored list by list;
 * ids int32 [G]: the original row of each stored row, ascending within a list; list_start int32 [L + 1].  probes int32
 * [Q, nprobe]: the lists query q walks; -1 (or any value outside [0, L)) is none, the other entries of a row must be distinct.
 * s, sc, the key bits(2 (1 - sc)) << 32 | ORIGINAL row, the order and dist are fn_gallery_search's bit for bit; rows int32 [Q, k]
 * holds original rows and skip int32 [Q] (or NULL) names one; a query with fewer than k admissible rows in its lists gets row -1,
 * dist +inf in the tail.  Given the index the result depends on nothing else; with every list probed it is fn_gallery_search's on
 * the unpermuted gallery.  range (2 words or NULL): ordered-int min/max of s over the pairs evaluated, skipped pairs included.
 * queries, lists and the workspace 16-byte aligned; 1 <= k <= 64; E a multiple of 4 in [4, 512]; L <= 2^20; Q nprobe <= 2^28.
 * workspace: at least the bytes fn_ivf_search_workspace reports for the same Q, L, nprobe, E and k (it holds one copy of a query
 * row and one k-list per (query, probe) pair).  The caller owns every buffer; no call here allocates or synchronises. */
int fn_kmeans_update(const float* rows, int N, int E, const int32_t* order, const int32_t* list_start, int L, const float* prev,
                     float* centroids, int32_t* kept, void* stream);
int fn_ivf_search_workspace(int Q, int L, int nprobe, int E, int k, long long* bytes);
int fn_ivf_search(const float* queries, int Q, const float* lists, const int32_t* ids, int G, const int32_t* list_start, int L, int E,
                  const int32_t* probes, int nprobe, int k, int metric, const int32_t* skip, void* workspace, float* dist,
                  int32_t* rows, int32_t* range, void* stream);

/* ---- the quantised gallery: an int8 shortlist, the exact re-rank of it and a certificate ---------------------
 * fn_quantize_rows: rows fp32 [N, E] (E a multiple of 4 in [4, 512]) -> codes int8 [N, Ep], Ep = E rounded up to a multiple of 64,
 * the padding zero; scale, rho, norm fp32 [N].  Per row x: m = max |x_e|; codes[e] = rint((double) x_e * 127.0 / (double) m) in
 * fp64, half to even (|code| <= 127); scale = (float)((double) m / 127.0); m = 0 gives codes and scale 0.  rho = ||x - scale c||:
 * the sequential fp64 sum from 0.0 over ascending e of t * t, t = (double) x_e - (double) scale * c_e, every product rounded
 * before it is used (no fused multiply-add), the IEEE square root, stored as the smallest float not below it; norm = ||x|| the
 * same way.  rows and codes 16-byte aligned.
 *
 * fn_qgallery_search: the k nearest of G gallery rows through a shortlist of R = shortlist rows, k <= R <= 64.  queries, gallery,
 * E, metric, skip, slab_rows and the alignment rule: as fn_gallery_search; qcodes / qscale / qrho / qnorm and gcodes / gscale: what
 * fn_quantize_rows gave for the two tables (code tables 16-byte aligned); rho_max, norm_max: the maxima of the gallery's rho and
 * norm.  Stage one (v_mfma_i32_16x16x64_i8): idot = the int32 dot product of two code rows, s^ = (qscale gscale) (float) idot
 * (two fp32 products in that association), key = bits(2 (1 - clip(s^))) << 32 | row; the shortlist is the R smallest keys,
 * ascending, skip[q] left out; shortlist_keys uint64 [Q, R] or NULL receives it, all ones behind its length.  Stage two: the
 * rows of the shortlist are ranked by fn_gallery_search's own key (the fp32 chain on queries and gallery) and cut to k: dist fp32
 * [Q, k], rows int32 [Q, k], row -1 and dist +inf in the tail.  certified int32 [Q]: 1 when the shortlist is not full, or when,
 * in fp64 and in this order, with u = 2^-24, g = E u / (1 - E u), B = qrho norm_max + (qnorm + qrho) rho_max + g qnorm norm_max
 * + 4 u:  (qnorm + qrho) (norm_max + rho_max) <= 1.05  and  d0_k < d~_R - 2 B - 8 u  (d0_k the k-th distance of stage two for
 * metric 0, d~_R the R-th of stage one).  A certified query's dist and rows are fn_gallery_search's bit for bit; any other query's
 * are the best k of its shortlist.  range (2 words or NULL): ordered-int min/max of the chain values s of the pairs re-ranked,
 * NOT of all Q x G pairs.  workspace: at least the bytes fn_qgallery_search_workspace reports for the same Q, G, k, shortlist and
 * slab_rows.  The result depends neither on slab_rows nor on scheduling.  The caller owns every buffer; no call here allocates or
 * synchronises. */
int fn_quantize_rows(const float* rows, int N, int E, int8_t* codes, float* scale, float* rho, float* norm, void* stream);
int fn_qgallery_search_workspace(int Q, int G, int k, int shortlist, int slab_rows, long long* bytes);
int fn_qgallery_search(const float* queries, int Q, const float* gallery, int G, const int8_t* qcodes, const float* qscale,
                       const int8_t* gcodes, const float* gscale, const float* qrho, const float* qnorm, double rho_max,
                       double norm_max, int E, int k, int shortlist, int metric, const int32_t* skip, int slab_rows, void* workspace,
                       float* dist, int32_t* rows, int32_t* certified, unsigned long long* shortlist_keys, int32_t* range,
                       void* stream);

/* ---- open-set 1:N evaluation: per probe its nearest mate, its nearest impostor and the rank of that mate;
 * the [Q, G] matrix never reaches memory.  s, sc, d0 = 2 (1 - sc) and the key bits(d0) << 32 | row are those of fn_gallery_search,
 * fn_radius_*, fn_confidence_counts* and fn_pair_key_histogram bit for bit.  queries, gallery, E, metric, skip, slab_rows and the
 * alignment rule: as fn_gallery_search.  query_labels int32 [Q] (>= -1) and gallery_labels int32 [G] (>= 0) must be given; the
 * caller guarantees their ranges.  Gallery row g is admissible for query q when g != skip[q]; an admissible row is a mate when
 * gallery_labels[g] == query_labels[q] and an impostor otherwise; a query label of -1 is a probe known to be absent: every row is
 * its impostor.  rows int32 [Q, 2]: the mate / the impostor with the smallest key (equal distances go to the lower row); dist fp32
 * [Q, 2]: that row's distance in the gallery's metric (2 (1 - sc) for metric 0, acosf(sc) for metric 1); row -1 and dist +inf
 * where there is no such row.  rank int32 [Q] or NULL: the number of admissible impostor rows whose key is smaller than the
 * nearest mate's, i.e. the 0-based rank of the first mate in the full ordering, -1 without a mate; it costs a second walk of the
 * gallery, which NULL leaves out.  range (2 words or NULL): ordered-int min/max of s over all Q x G pairs, skipped pairs
 * included.  workspace: at least the bytes fn_mate_search_workspace reports for the same Q, G and slab_rows.  The result depends
 * neither on slab_rows nor on scheduling.  There is no small-Q mode: this is an evaluation over many probes.  The caller owns
 * every buffer; the call allocates nothing and does not synchronise. */
int fn_mate_search_workspace(int Q, int G, int slab_rows, long long* bytes);
int fn_mate_search(const float* queries, int Q, const int32_t* query_labels, const float* gallery, int G,
                   const int32_t* gallery_labels, int E, int metric, const int32_t* skip, int slab_rows, void* workspace,
                   float* dist, int32_t* rows, int32_t* rank, int32_t* range, void* stream);

/* ---- candidate lists of identities: per query the k nearest DISTINCT labels, each through its nearest row;
 * the [Q, G] matrix never reaches memory.  s, sc, d0 = 2 (1 - sc) and the key bits(d0) << 32 | row are those of fn_gallery_search
 * bit for bit.  queries, gallery, E, metric, skip, slab_rows and the alignment rule: as fn_gallery_search.  gallery_labels int32
 * [G] (>= 0) must be given; the caller guarantees the range.  Gallery row g is admissible for query q when g != skip[q].  For a
 * label c, best(q, c) is the smallest key over the admissible rows with gallery_labels[g] == c.  The result for q is the k labels
 * with the smallest best, ascending by best: rows int32 [Q, k] holds the row in that key (the identity's nearest row, equal
 * distances going to the lower row), dist fp32 [Q, k] that row's distance in the gallery's metric (2 (1 - sc) for metric 0,
 * acosf(sc) of the recomputed chain for metric 1).  A query with fewer than k admissible identities gets row -1 and dist +inf in
 * the tail.  1 <= k <= 64.  range (2 words or NULL): ordered-int min/max of s over all Q x G pairs, skipped pairs included.
 * workspace: at least the bytes fn_gallery_candidates_workspace reports for the same Q, G, k and slab_rows: slabs x lists x Q x k
 * 8-byte keys, slabs = ceil(G / slab_rows rounded up to a multiple of 64), lists = 4 for Q <= 16 and 1 otherwise.  The result
 * depends neither on slab_rows nor on scheduling.  The caller owns every buffer; the call allocates nothing and does not
 * synchronise. */
int fn_gallery_candidates_workspace(int Q, int G, int k, int slab_rows, long long* bytes);
int fn_gallery_candidates(const float* queries, int Q, const float* gallery, int G, const int32_t* gallery_labels, int E, int k,
                          int metric, const int32_t* skip, int slab_rows, void* workspace, float* dist, int32_t* rows, int32_t* range,
                          void* stream);

/* ---- face clustering ------------------------------------------------------------------------------------
 * Radius search: every (query, gallery row) pair with d < eps as a CSR; the [Q, G] matrix never reaches memory.  s, sc and d
 * (2 (1 - sc) for metric 0, acosf(sc) for metric 1) are those of fn_gallery_search and fn_confidence_counts bit for bit, and the
 * comparison is the strict fp32 <.  queries, gallery, E, skip, slab_rows and the alignment rule: as fn_gallery_search.
 * fn_radius_count: offsets int64 [Q + 1] receives the exclusive scan of the rows' neighbour counts (offsets[Q] = nnz); range
 *   (2 words or NULL): ordered-int min/max of s over all Q x G pairs.  The workspace (fn_radius_workspace bytes for the same Q, G,
 *   slab_rows) keeps where every (slab, query) writes and goes unchanged to
 * fn_radius_fill with the same queries, gallery, metric, eps, skip and slab_rows: cols int32 / dist fp32 [capacity] receive each
 *   row's neighbours in ascending column order (the CSR does not depend on slab_rows).  Nothing is written at or beyond
 *   `capacity`; it should be offsets[Q], which the caller reads between the two calls.
 * Neither call allocates or synchronises.
 *
 * DBSCAN on the self-join CSR (Q = G = N, skip[i] = i): a row is a core row when degree + 1 >= min_samples; clusters are the
 * connected components of the core rows; a non-core row with a core neighbour joins the cluster of the core neighbour with the
 * smallest (bits(d0) << 32 | col) key, d0 the metric-0 distance; every other row is noise, label -1; ids 0 .. C - 1 ascend with
 * each cluster's smallest core row.
 * fn_dbscan_init: core int32 [N], labels int32 [N] (the working forest until fn_dbscan_finish), info int32 [8] = {converged,
 *   rounds run, clusters, noise rows, 4 words of the library's}.
 * fn_dbscan_rounds: enqueues `rounds` (1 .. 1024) rounds of hooking to the minimum label + pointer jumping; a round does
 *   nothing once info[0] is set.  The caller reads info[0] and repeats while it is 0.
 * fn_dbscan_finish, once, after convergence: border rows, consecutive ids, info[2], info[3].  ids: int32 [N] scratch.  metric 0:
 *   dist IS d0 and emb may be NULL; metric 1: d0 is recomputed from emb fp32 [N, E] (the same fmaf chain).
 * None of the three allocates or synchronises. */
int fn_radius_workspace(int Q, int G, int slab_rows, long long* bytes);
int fn_radius_count(const float* queries, int Q, const float* gallery, int G, int E, int metric, float eps, const int32_t* skip,
                    int slab_rows, void* workspace, int64_t* offsets, int32_t* range, void* stream);
int fn_radius_fill(const float* queries, int Q, const float* gallery, int G, int E, int metric, float eps, const int32_t* skip,
                   int slab_rows, const void* workspace, int32_t* cols, float* dist, long long capacity, void* stream);
int fn_dbscan_init(int N, const int64_t* offsets, int min_samples, int32_t* labels, int32_t* core, int32_t* info, void* stream);
int fn_dbscan_rounds(int N, const int64_t* offsets, const int32_t* cols, const int32_t* core, int32_t* labels, int32_t* info,
                     int rounds, void* stream);
int fn_dbscan_finish(int N, const int64_t* offsets, const int32_t* cols, const float* dist, int metric, const float* emb, int E,
                     const int32_t* core, int32_t* labels, int32_t* ids, int32_t* info, void* stream);

/* ---- hierarchical clustering: the minimum spanning tree of N rows under the mutual-reachability distance,
 * by Boruvka's algorithm on the device; the [N, N] matrix never reaches memory.  s and d = 2 (1 - sc) are those of fn_gallery_search,
 * fn_radius_* and fn_mate_search bit for bit (metric 0 only: acosf is not pinned bit for bit, and the tree is).  The weight of the
 * pair (i, j) is w = max(d(i, j), core[i], core[j]) in fp32; core fp32 [N] or NULL (zeros).  Edges are ordered by (bits(w), lo, hi),
 * lo = min(i, j), hi = max(i, j); the result is THE minimum spanning tree under that strict total order (Kruskal's on the edges
 * sorted that way), so it depends neither on slab_rows nor on scheduling.  rows fp32 [N, E], E, slab_rows and the alignment rule:
 * as fn_mate_search's gallery.
 * fn_mst_init: comp int32 [N] = 0 .. N - 1 (a row's component: the smallest row of it), info int32 [8] = {done, rounds run,
 *   components, edges written, 4 words of the library's}.  N = 1 is done at once.
 * fn_mst_rounds: enqueues `rounds` (1 .. 64) rounds: one walk of all pairs that finds every row's nearest row of another
 *   component, then the contraction.  A round at least halves the components, so ceil(log2 N) rounds finish; a round does nothing
 *   once info[0] is set, so the caller may enqueue them all and read info once.  edges int32 [N - 1][2] (lo < hi) and weights fp32
 *   [N - 1] receive the tree; the SET of edges is the contract, their order in the buffer is not.  workspace: at least the bytes
 *   fn_mst_workspace reports for the same N and slab_rows, the same buffer for every call of one tree.
 * No call allocates or synchronises. */
int fn_mst_workspace(int N, int slab_rows, long long* bytes);
int fn_mst_init(int N, int32_t* comp, int32_t* info, void* stream);
int fn_mst_rounds(const float* rows, int N, int E, const float* core, int slab_rows, void* workspace, int32_t* comp, int32_t* edges,
                  float* weights, int32_t* info, int rounds, void* stream);

/* ---- softmax classifier loss: apps/train_softmax.py:91 (SparseCategoricalCrossentropy(from_logits)); loss: fp32[4] as above;
 * dbias (optional): fixed point, FN_ACC_GRAD_BITS, += column sums of dlogits */
int fn_softmax_xent_fwd_bwd(const float* logits, int ld, const int32_t* labels, float* loss, void* dlogits_lp, int ld_d, fn_acc_t* dbias, int N,
                            int C, float grad_scale, int dtype, void* stream);

/* ---- large-margin cosine softmax: NormFace / CosFace / ArcFace ------------------------------------------
 * The classifier runs on the L2-normalised embedding; z = xhat . w_j comes from fn_conv2d_fwd without bias.
 * fn_margin_weight_rnorm: rnorm[j] = 1 / sqrt(max(sum_e w[j][e]^2, eps)) for the C rows of fp32 w [C][E] (E % 4 == 0, w 16-byte
 *   aligned); a one-hot row gives exactly 1.
 * fn_margin_softmax_fwd_bwd: c = clamp(z rnorm, -1, 1); in the label's column ct = clamp(c, -T, T), T = 1 - 2^-20, and
 *   phi = ct cos m_arc - sqrt((1 - ct)(1 + ct)) sin m_arc - m_cos if ct > cos(pi - m_arc), else ct - sin(pi - m_arc) m_arc - m_cos;
 *   logits l = scale c (scale phi in the label's column); loss (fp32[4] as above) = mean_i (logsumexp l_i - l_i[label]);
 *   g = scale (softmax(l) - onehot) grad_scale D with D = dphi/dc at ct in the label's column (1 on the linear branch) and 1
 *   elsewhere: both clamps are straight-through.  dz_lp (optional) [N][ld_d] = g rnorm in low precision, columns C..ld_d zero;
 *   t (optional, fixed point, FN_ACC_GRAD_BITS) t[c] += sum_i g c.  Columns >= C of z and rnorm are never read.  A label outside
 *   [0, C) gives a NaN loss and no one-hot term.  scale > 0, 0 <= m_arc < pi/2, m_cos >= 0, else FN_EINVAL.
 * fn_margin_wgrad_fix: the gradient through the row normalisation, dw[j][e] -= rnorm[j]^2 t[j] w[j][e] for j < C (dw, w fp32
 *   [.][E], 16-byte aligned, E % 4 == 0); t[0..C) is read and left zeroed for the next step. */
int fn_margin_weight_rnorm(const float* w, int C, int E, float eps, float* rnorm, void* stream);
int fn_margin_softmax_fwd_bwd(const float* z, int ld, const float* rnorm, const int32_t* labels, float* loss, void* dz_lp, int ld_d,
                              fn_acc_t* t, int N, int C, float scale, float m_arc, float m_cos, float grad_scale, int dtype, void* stream);
int fn_margin_wgrad_fix(float* dw, const float* w, const float* rnorm, fn_acc_t* t, int C, int E, void* stream);

/* ---- embedding regularisers of softmax training ------------------------------------------------------
 * fn_center_loss_fwd_bwd: center loss of facenet/facenet.py:204-217 (center_loss) and the prelogits-norm loss named by
 * loss.prelogits_norm_factor / prelogits_norm_p of apps/configs/train_softmax.yaml:73-78, one launch (+ a one-thread finish).
 * x fp32 [N,E] (E % 4 == 0; x, demb, centers 16-byte aligned), labels int32 [N], centers fp32 [C,E] or NULL (no center term).
 *   terms: fp32[8], 8-byte aligned, ZEROED ONCE by the caller (every call leaves words 2..7 zeroed again).  word 0 receives
 *   center_loss = mean_{i,e} (x - centers[label])^2 (unset without centers; NaN for a non-finite term / a label outside [0, C)),
 *   word 1 prelogits_norm = mean_i (sum_e (|x|+1e-4)^p)^(1/p) (NaN for a non-finite term).
 *   demb (optional) fp32 [N,E] += center_factor * 2 (x - c)/(N E) + norm_factor * sign(x) a^(p-1) n_i^(1-p) / N; a term whose
 *   factor is 0 adds nothing.  xy (optional) [N][ld_xy] receives x (E values) and float(label) at column E: the rows
 *   fn_center_update reads.
 * fn_center_update: facenet.py:212-213 (scatter_sub of (1 - alfa)(centers[label] - x)) in a fixed order: per class, the rows that
 *   carry it in ascending row order, c <- c - k (c_old - x_j), k = float(1 - alfa).  rows [M][ld] as written by the above (M <= 4096;
 *   under data parallelism the gathered global batch in rank order); rows whose label is not an integer in [0, C) are skipped. */
int fn_center_loss_fwd_bwd(const float* x, const int32_t* labels, const float* centers, float* demb, float* terms, float* xy, int ld_xy,
                           int N, int E, int C, float center_factor, float norm_factor, float p, void* stream);
int fn_center_update(const float* rows, int ld, int M, int E, float* centers, int C, double alfa, void* stream);

/* ---- face-to-face pair classifiers ---------------------------------------------------------------------
 * facenet/faceclass.py:8-118: d(x, y) = 2 (1 - x.y / (|x| |y|)) + theta (2 (|x| - |y|) / (|x| + |y|))^2 (mode 0, distance
 * classifier) or 2 (1 - x.y) (mode 1, normalized classifier); logits = alpha (threshold - d); predict = d < threshold.
 * Tables fp32 [n][E], E % 4 == 0, 16-byte aligned.  params: device fp32[4] = {alpha, threshold, theta, 0}, read on the device
 * (graph replays see the optimiser's updates).  norms = fn_f2f_row_norms of the same table; NULL allowed in mode 1 only.  The
 * three pair entry points share one per-pair distance function: their distances agree bit for bit.
 * fn_f2f_row_norms: norms[r] = |x_r| (fp64 sum of squares, rounded once).
 * fn_f2f_pair_loss_fwd_bwd: apps/train_classifier.py:60-84 (binary_cross_entropy_loss) + its gradient.  Batch row b is table
 *   row rows[b] (device int32 [P K], grouped by class: z = (a / K == b / K)); pairs a < b; weighted_cross_entropy_with_logits with
 *   pos_weight q.  loss: fp32[1] = mean over the pairs; grad: fp32[4] = dL/d{alpha, threshold, theta, 0} (theta's is 0 in mode 1),
 *   the g of fn_adam_keras with n = 4.  ws: fp64 workspace of >= 4 T doubles, T = nt (nt + 1) / 2, nt = ceil(P K / 64) (one slot
 *   per upper-triangle 64 x 64 tile, summed in tile order: same bits every run; a NaN embedding gives a NaN loss and gradient).
 *   An index outside [0, n_rows) reads as a NaN row.
 * fn_f2f_pair_counts: apps/train_classifier.py:27-39 (ConfusionMatrix: classifier.predict for every class pair).  Class c =
 *   table rows cls_start[c] .. cls_start[c+1] (device int32 [C+1]); counts int64 [C (C+1) / 2], slot i (i+1)/2 + k for k <= i,
 *   receives #(d < threshold) over the whole n_i x n_k rectangle (the whole square, diagonal included, for k == i).
 * fn_f2f_distance: faceclass.py:45-77 / :102-110 (distance) or :23-27 (__call__, logits != 0): out fp32 [N, M] for x [N, E],
 *   y [M, E] (y == x for the reference's y=None). */
int fn_f2f_row_norms(const float* x, int n, int E, float* norms, void* stream);
int fn_f2f_pair_loss_fwd_bwd(const float* table, const float* norms, int n_rows, const int32_t* rows, int P, int K, int E, int mode,
                             float q, const float* params, float* loss, float* grad, double* ws, long ws_len, void* stream);
int fn_f2f_pair_counts(const float* table, const float* norms, const int32_t* cls_start, int C, int E, int mode, const float* params,
                       int64_t* counts, void* stream);
int fn_f2f_distance(const float* x, const float* nx, int N, const float* y, const float* ny, int M, int E, int mode, const float* params,
                    int logits, float* out, void* stream);

/* ---- optimiser: tf.keras.optimizers.Adam(epsilon=0.1) apps/train_softmax.py:92 + Keras L2(5e-4) (:65) ----
 * hyper = device word[8] {lr, beta1^t, beta2^t, grad_scale, t (int32: Keras' `iterations`), 3 spare}; fn_adam_tick advances t and
 * re-derives the beta powers from it on the device (graph replay safe; t survives past the fp32 underflow of beta1^t).
 * Elements [0, n_decay) get the coupled L2 term g += 2*l2*w.  w_lp receives the low-precision copy of w[0, n_lp).
 * n > 0, n % 4 == 0, 0 <= n_decay <= n, 0 <= n_lp <= n, n_lp % 4 == 0, else FN_EINVAL. */
int fn_adam_keras(float* w, const float* g, float* m, float* v, void* w_lp, long n_lp, long n, long n_decay, float* hyper, float beta1,
                  float beta2, float eps, float l2, int dtype, void* stream);
/* fn_adam_keras_ema: fn_adam_keras (w, m, v, w_lp bit-identical) fused with the moving average of the new weights over [0, n):
 * shadow = shadow - (shadow - w) * (1 - d), d = fminf(decay, (1 + t) / (10 + t)), t = word 4 of hyper; decay in (0, 1). */
int fn_adam_keras_ema(float* w, const float* g, float* m, float* v, void* w_lp, long n_lp, long n, long n_decay, float* hyper,
                      float beta1, float beta2, float eps, float l2, int dtype, float* shadow, float decay, void* stream);
int fn_adam_tick(float* hyper, float beta1, float beta2, void* stream);
/* fn_opt_keras: the other update rules of train.optimizer, the Keras optimizers of the TF1 names, in one
 * fused pass with the g, hyper (lr = word 0, grad_scale = word 3), n_decay and w_lp pack of fn_adam_keras.  rule = FN_OPT_*:
 *   FN_OPT_ADAGRAD  s1 = accumulator                      a += g^2; w -= lr g / (sqrt(a) + eps)
 *   FN_OPT_ADADELTA s1 = accum_grad, s2 = accum_var       ag = rho ag + (1-rho) g^2; u = sqrt(av+eps) / sqrt(ag+eps) g; w -= lr u;
 *                                                         av = rho av + (1-rho) u^2
 *   FN_OPT_RMSPROP  s1 = rms, s2 = momentum               ms = rho ms + (1-rho) g^2; mom = momentum mom + lr g / sqrt(ms+eps); w -= mom
 *   FN_OPT_MOM      s1 = momentum (Nesterov)              acc = momentum acc - lr g; w += momentum acc - lr g
 * Unused constants are ignored; s2 may be null for the one-slot rules.  fn_adam_tick still advances t (word 4) once per step.
 * fn_opt_keras_ema: the same pass (w, slots, w_lp bit-identical) fused with the moving average of fn_adam_keras_ema. */
#define FN_OPT_ADAGRAD 1
#define FN_OPT_ADADELTA 2
#define FN_OPT_RMSPROP 3
#define FN_OPT_MOM 4
int fn_opt_keras(int rule, float* w, const float* g, float* s1, float* s2, void* w_lp, long n_lp, long n, long n_decay, float* hyper,
                 float rho, float momentum, float eps, float l2, int dtype, void* stream);
int fn_opt_keras_ema(int rule, float* w, const float* g, float* s1, float* s2, void* w_lp, long n_lp, long n, long n_decay, float* hyper,
                     float rho, float momentum, float eps, float l2, int dtype, float* shadow, float decay, void* stream);

/* ---- weight packs ----------------------------------------------------------------------------------
 * table = device int32 [n_layers][8] {w_off, cout, ktot, taps, cin, bn_off(-1 none), fold_bias_off, 0}.
 * fn_pack_transpose: wt[cin][tap][cout] = w[cout][tap][cin] (dgrad operand) for every layer.
 * fn_fold_bn: wf = lp(w * rsqrt(var+eps)[cout]), bias = beta - mean*rsqrt(var+eps)   (facenet/tfutils.py:244-250)
 * Every row: w_off and cin multiples of 8, ktot == taps * cin (the 16-byte paths; not checkable here: the table is device
 * memory); fn_pack_transpose moves a layer whose cout is no multiple of 8 element by element.  n_layers > 0 and
 * max_layer_elems > 0 (it sizes the grid), else FN_EINVAL. */
int fn_pack_transpose(const void* w_lp, void* wt_lp, const int32_t* table, int n_layers, int max_layer_elems, int dtype, void* stream);
int fn_fold_bn(const float* w, void* wf_lp, float* fold_bias, const float* beta, const float* moving_mean, const float* moving_var,
               const int32_t* table, int n_layers, int max_layer_elems, float eps, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
