// Training-time augmentation of the input pipeline (image.random_rotate / random_crop / random_flip of
// apps/configs/train_softmax.yaml:85-91; semantics in DESIGN.md section 13, restated in tests/augment_oracle.py).  For one
// ragged batch of decoded HWC u8 images (the packing of fn_crop_or_pad_u8) and one fn_augment_param per image, every output
// pixel is produced in one pass: flip -> crop/pad offset -> rotated bilinear sample of the source.  No rotated intermediate is
// written and no atomics are used.  An image whose (sin, cos) is (0, 1) takes a pure byte-copy path, so all keys off equals
// fn_crop_or_pad_u8 byte for byte.  fn_resident_batch_u8 is the same pass over a data set that lives in device memory: its
// images are addressed by row number through the store's own tables.
#include "common.h"
#include "../../include/facenet_hip.h"

namespace fn {

// u8 tap of image `im` (h x w x 3) at (y, x), 0 outside
__device__ __forceinline__ float aug_tap(const uint8_t* im, int h, int w, int y, int x, int c) {
    return (y >= 0 && y < h && x >= 0 && x < w) ? (float)im[((long)y * w + x) * 3 + c] : 0.f;
}

// Rotated image R at integer (ry, rx): bilinear sample of the source at the rotated point, every rounding spelled out (the oracle
// repeats this order in float32).
__device__ __forceinline__ void aug_rotated(const uint8_t* im, int h, int w, float hw2, float hh2, float cs, float sn, int ry, int rx,
                                           uint8_t* out) {
#pragma clang fp contract(off)
    const float u = ((float)rx + 0.5f) - hw2, v = ((float)ry + 0.5f) - hh2;
    const float sx = ((cs * u - sn * v) + hw2) - 0.5f;
    const float sy = ((sn * u + cs * v) + hh2) - 0.5f;
    const float flx = floorf(sx), fly = floorf(sy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float fx = sx - flx, fy = sy - fly;
    const float gx = 1.f - fx, gy = 1.f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = gx * aug_tap(im, h, w, y0, x0, c) + fx * aug_tap(im, h, w, y0, x0 + 1, c);
        const float bot = gx * aug_tap(im, h, w, y0 + 1, x0, c) + fx * aug_tap(im, h, w, y0 + 1, x0 + 1, c);
        const float r = rintf(gy * top + fy * bot);
        out[c] = (uint8_t)(int)fminf(fmaxf(r, 0.f), 255.f);
    }
}

// Output quad q of one image = 4 output pixels = 12 bytes = three 32-bit stores (S even, so S*S % 4 == 0 and every quad is 4-byte
// aligned).  Source bytes are unaligned gathers, read through L1 as in crop_or_pad_kernel.  `copy` is per image, so it is uniform
// across a block.  The one definition of the per-pixel work: augment_kernel and resident_batch_kernel differ only in where `im`,
// (h, w) and the record come from.
__device__ __forceinline__ void aug_quad(const uint8_t* im, int h, int w, const fn_augment_param& p, bool copy, float hw2, float hh2,
                                         int S, int q, unsigned* out) {
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pix = q * 4 + k;
        const int y = pix / S, x = pix % S;
        const int ry = y + p.y0, rx = (p.flip ? S - 1 - x : x) + p.x0;
        uint8_t* o = px + 3 * k;
        o[0] = o[1] = o[2] = 0;
        if (ry < 0 || ry >= h || rx < 0 || rx >= w) continue;       // padding (R has the source's size)
        if (copy) {
            const uint8_t* s = im + ((long)ry * w + rx) * 3;
            o[0] = s[0], o[1] = s[1], o[2] = s[2];
        } else {
            aug_rotated(im, h, w, hw2, hh2, p.cos_t, p.sin_t, ry, rx, o);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        out[3 * q + j] = (unsigned)px[4 * j] | (unsigned)px[4 * j + 1] << 8 | (unsigned)px[4 * j + 2] << 16 |
                         (unsigned)px[4 * j + 3] << 24;
}

// One thread per quad, blockIdx.y = image.
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ off,
                                                      const int* __restrict__ hw, const fn_augment_param* __restrict__ prm,
                                                      uint8_t* __restrict__ dst, int S) {
    const int n = blockIdx.y;
    const int h = hw[2 * n], w = hw[2 * n + 1];
    const fn_augment_param p = prm[n];
    const bool copy = p.sin_t == 0.f && p.cos_t == 1.f;
    const float hw2 = 0.5f * (float)w, hh2 = 0.5f * (float)h;      // exact: w, h < 2^24
    const uint8_t* im = src + off[n];
    unsigned* out = reinterpret_cast<unsigned*>(dst + (long)n * S * S * 3);
    const int quads = S * S / 4;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) aug_quad(im, h, w, p, copy, hw2, hh2, S, q, out);
}

// The same batch built from a resident store: image n of the batch is row rows[n] of the data set's own offset / (h, w) tables,
// so nothing is gathered per batch.  prm == nullptr: the centre crop / pad record of fn_crop_or_pad_u8, made here from (h, w).
// A row outside [0, M) reads neither table nor pool and gives an all-zero image (the row is uniform across the block).
__global__ __launch_bounds__(256) void resident_batch_kernel(const uint8_t* __restrict__ pool, const long long* __restrict__ off,
                                                             const int* __restrict__ hw, long long M, const int* __restrict__ rows,
                                                             const fn_augment_param* __restrict__ prm, uint8_t* __restrict__ dst, int S) {
    const int n = blockIdx.y;
    const long long r = rows[n];
    unsigned* out = reinterpret_cast<unsigned*>(dst + (long)n * S * S * 3);
    const int quads = S * S / 4;
    if (r < 0 || r >= M) {
        for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) out[3 * q] = out[3 * q + 1] = out[3 * q + 2] = 0u;
        return;
    }
    const int h = hw[2 * r], w = hw[2 * r + 1];
    fn_augment_param p;
    if (prm) {
        p = prm[n];
    } else {                                                        // offset_crop = (h - S) / 2, offset_pad = (S - h) / 2
        p.y0 = h > S ? (h - S) / 2 : -((S - h) / 2);
        p.x0 = w > S ? (w - S) / 2 : -((S - w) / 2);
        p.flip = 0, p.cos_t = 1.f, p.sin_t = 0.f;
    }
    const bool copy = p.sin_t == 0.f && p.cos_t == 1.f;
    const float hw2 = 0.5f * (float)w, hh2 = 0.5f * (float)h;
    const uint8_t* im = pool + off[r];                             // 64-bit byte offset: a pool is tens of GB
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) aug_quad(im, h, w, p, copy, hw2, hh2, S, q, out);
}

extern "C" int fn_augment_u8(const uint8_t* src, const long long* offsets, const int32_t* hw, const fn_augment_param* params, uint8_t* dst,
                             int N, int S, void* stream) {
    FN_REQUIRE(src && offsets && hw && params && dst && N > 0 && N <= 65535 && S > 0 && S % 2 == 0 && S <= 16384,
               "augment: bad arguments");
    hipLaunchKernelGGL(augment_kernel, dim3(cdiv((long)S * S / 4, 256), N), dim3(256), 0, (hipStream_t)stream, src, offsets, hw, params, dst, S);
    return check_launch("augment");
}

extern "C" int fn_resident_batch_u8(const uint8_t* pool, const long long* offsets, const int32_t* hw, long long M, const int32_t* rows,
                                    const fn_augment_param* params, uint8_t* dst, int N, int S, void* stream) {
    FN_REQUIRE(pool && offsets && hw && rows && dst && M > 0 && N > 0 && N <= 65535 && S > 0 && S % 2 == 0 && S <= 16384,
               "resident_batch: bad arguments");
    hipLaunchKernelGGL(resident_batch_kernel, dim3(cdiv((long)S * S / 4, 256), N), dim3(256), 0, (hipStream_t)stream, pool, offsets, hw, M,
                       rows, params, dst, S);
    return check_launch("resident_batch");
}

}  // namespace fn
