// Landmark alignment of detected faces on the device (restated in tests/align_oracle.py): every face of one
// frame is warped through its own inverse similarity transform onto an S x S output, bilinear taps with a constant-zero border
// under an n x n box prefilter (n sub-samples per axis, 1 .. 8, chosen per face by the host from the transform's scale).  The fit
// of the transform to the five landmarks is host arithmetic (facenet_amd/detectors/face_detector.py); this file is the warp.
//
// One launch per batch: grid (16 x 16-pixel tiles, F), one thread per output pixel and all three channels.  Everything is fp64
// in the definition's order without contraction, so the bytes equal the NumPy oracle's bit for bit.
#include <math.h>

#include "common.h"
#include "../../include/facenet_hip.h"

#pragma clang fp contract(off)      // the oracle's doubles, rounding by rounding: no fused multiply-add anywhere in this file

namespace fn {

enum { FA_TILE = 16 };              // 16 x 16 output pixels per workgroup: 100 workgroups for one face at S = 160

// One tap: the pixel at (x, y) or zeros outside the frame.  The index is clamped into the frame before the address is formed,
// so the load itself is always inside [0, H) x [0, W).
__device__ __forceinline__ void fa_tap(const uint8_t* __restrict__ frame, int H, int W, int x, int y, double& c0, double& c1, double& c2) {
    const bool inside = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
    const int xc = min(max(x, 0), W - 1), yc = min(max(y, 0), H - 1);
    const uint8_t* p = frame + ((long)yc * W + xc) * 3;
    const uint8_t r = p[0], g = p[1], b = p[2];
    c0 = inside ? (double)r : 0.0, c1 = inside ? (double)g : 0.0, c2 = inside ? (double)b : 0.0;
}

__device__ __forceinline__ uint8_t fa_round8(double acc, double count) {
    const double v = rint(acc / count);          // round half to even
    return (uint8_t)(v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v);
}

// workspace: inverse double [F][6] | samples int32 [F]
__global__ __launch_bounds__(FA_TILE * FA_TILE) void face_align_kernel(const uint8_t* __restrict__ frame, int H, int W,
                                                                      const double* __restrict__ inverse, const int32_t* __restrict__ samples,
                                                                      int S, int tiles_x, uint8_t* __restrict__ dst) {
    __shared__ double offset[8];                 // (i + 0.5) / n - 0.5: where sub-sample i lies within its output pixel
    const int f = blockIdx.y;
    const int n = min(max(samples[f], 1), 8);    // the host checked 1 .. 8; the clamp keeps the table inside its 8 entries regardless
    if (threadIdx.x < 8) offset[threadIdx.x] = ((double)threadIdx.x + 0.5) / (double)n - 0.5;
    __syncthreads();
    const int u = blockIdx.x % tiles_x * FA_TILE + threadIdx.x % FA_TILE;
    const int v = blockIdx.x / tiles_x * FA_TILE + threadIdx.x / FA_TILE;
    if (u >= S || v >= S) return;
    const double* m = inverse + 6 * (long)f;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const double xlim = (double)(W - 1), ylim = (double)(H - 1);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int j = 0; j < n; ++j) {
        const double vv = (double)v + offset[j];
        for (int i = 0; i < n; ++i) {
            const double uu = (double)u + offset[i];
            const double x = (m0 * uu + m1 * vv) + m2, y = (m3 * uu + m4 * vv) + m5;
            const double xf = floor(x), yf = floor(y);
            // all four taps outside the frame: the sample is 0 and leaves the sums as they are (also keeps the int casts in range)
            if (!(xf >= -1.0 && xf <= xlim && yf >= -1.0 && yf <= ylim)) continue;
            const double fx = x - xf, fy = y - yf;
            const int x0 = (int)xf, y0 = (int)yf;
            double p00[3], p01[3], p10[3], p11[3];
            fa_tap(frame, H, W, x0, y0, p00[0], p00[1], p00[2]);
            fa_tap(frame, H, W, x0 + 1, y0, p01[0], p01[1], p01[2]);
            fa_tap(frame, H, W, x0, y0 + 1, p10[0], p10[1], p10[2]);
            fa_tap(frame, H, W, x0 + 1, y0 + 1, p11[0], p11[1], p11[2]);
            const double gx = 1.0 - fx, gy = 1.0 - fy;
            a0 += (p00[0] * gx + p01[0] * fx) * gy + (p10[0] * gx + p11[0] * fx) * fy;
            a1 += (p00[1] * gx + p01[1] * fx) * gy + (p10[1] * gx + p11[1] * fx) * fy;
            a2 += (p00[2] * gx + p01[2] * fx) * gy + (p10[2] * gx + p11[2] * fx) * fy;
        }
    }
    const double count = (double)(n * n);
    uint8_t* o = dst + (((long)f * S + v) * S + u) * 3;
    o[0] = fa_round8(a0, count), o[1] = fa_round8(a1, count), o[2] = fa_round8(a2, count);
}

static long long face_align_bytes(int F) { return (F * 52ll + 7) / 8 * 8; }      // 6 doubles + 1 int32 per face

extern "C" int fn_face_align_workspace(int F, long long* bytes) {
    FN_REQUIRE(bytes, "face_align_workspace: bad arguments");
    FN_REQUIRE(F > 0 && F <= 65535, "face_align: F = %d faces (1 .. 65535 expected)", F);
    *bytes = face_align_bytes(F);
    return FN_OK;
}

extern "C" int fn_face_align_u8(const uint8_t* frame, int H, int W, const double* inverse, const int32_t* samples, int F, int S, uint8_t* dst,
                                void* workspace, long long workspace_bytes, void* stream) {
    FN_REQUIRE(frame && inverse && samples && dst && workspace && H > 0 && W > 0 && (long)H * W * 3 < (1l << 40), "face_align: bad arguments");
    FN_REQUIRE(F > 0 && F <= 65535, "face_align: F = %d faces (1 .. 65535 expected)", F);
    FN_REQUIRE(S > 0 && S <= FN_FACE_ALIGN_MAX_SIDE, "face_align: side %d outside 1 .. %d", S, FN_FACE_ALIGN_MAX_SIDE);
    FN_REQUIRE(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= face_align_bytes(F), "face_align: workspace of %lld bytes, %lld 8-aligned needed",
               workspace_bytes, face_align_bytes(F));
    for (int f = 0; f < F; ++f) {
        FN_REQUIRE(samples[f] >= 1 && samples[f] <= FN_FACE_ALIGN_MAX_SAMPLES, "face_align: face %d takes %d sub-samples per axis (1 .. %d expected)", f,
                   samples[f], FN_FACE_ALIGN_MAX_SAMPLES);
        for (int k = 0; k < 6; ++k)      // a NaN fails the comparison too
            FN_REQUIRE(fabs(inverse[6 * f + k]) < 16777216.0, "face_align: face %d has the inverse entry %g (finite, below 2^24 expected)", f,
                       inverse[6 * f + k]);
    }
    hipStream_t st = (hipStream_t)stream;
    double* d_inverse = (double*)workspace;
    int32_t* d_samples = (int32_t*)(d_inverse + 6 * (long)F);
    if (hipMemcpyAsync(d_inverse, inverse, sizeof(double) * 6 * F, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_samples, samples, sizeof(int32_t) * F, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("face_align: copying the transforms to the device failed");
        return FN_ELAUNCH;
    }
    const int tiles_x = cdiv(S, FA_TILE);
    hipLaunchKernelGGL(face_align_kernel, dim3(tiles_x * tiles_x, F), dim3(FA_TILE * FA_TILE), 0, st, frame, H, W, d_inverse, d_samples, S, tiles_x, dst);
    return check_launch("face_align");
}

}  // namespace fn
