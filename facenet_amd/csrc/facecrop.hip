// Crop and resize detected faces on the device: PIL's `frame.crop(window).resize((side, side), LANCZOS)` for 8-bit RGB, bit for
// bit (Pillow's Resample.c; semantics in DESIGN.md section 17, restated in tests/face_crop_oracle.py).  Two launches per batch
// of windows over one frame:
//   1. face_taps_kernel: one thread per (face, axis, output index) computes Pillow's bounds and 22-bit fixed-point Lanczos taps
//      in fp64 into the caller's workspace, padded to the batch's largest tap count.
//   2. face_crop_kernel: one workgroup per (face, tile of output rows).  The horizontally filtered uint8 rows that the tile
//      needs go to LDS, the vertical pass reads them from there; the intermediate never reaches memory, and only the requested
//      output window (ox, oy, S) is computed.
// An axis whose crop extent equals `side` is a copy in Pillow; here it is the single tap 2^22 at the pixel itself, which the
// pass reproduces exactly ((2^21 + 2^22 p) >> 22 == p).
#include <math.h>

#include "common.h"
#include "../../include/facenet_hip.h"

#pragma clang fp contract(off)      // Pillow's doubles, rounding by rounding: no fused multiply-add anywhere in this file

namespace fn {

enum {
    FC_BITS = 22,                    // PRECISION_BITS of Resample.c for 8-bit channels
    FC_LDS_BYTES = 64 * 1024,        // static LDS of face_crop_kernel
    FC_MAX_TILE = 16,                // output rows per workgroup at most
};

// ---- the one definition of an axis' geometry, host and device ------------------------------------------------------------
struct AxisGeom {
    double scale, fs, support;
    int ksize;                       // Pillow's bound on the tap count: ceil(support) * 2 + 1
};
__host__ __device__ static inline AxisGeom axis_geom(int in_size, int side) {
    AxisGeom g;
    g.scale = (double)in_size / (double)side;
    g.fs = g.scale < 1.0 ? 1.0 : g.scale;
    g.support = 3.0 * g.fs;
    g.ksize = in_size == side ? 1 : (int)ceil(g.support) * 2 + 1;
    return g;
}

__device__ static inline double fc_sinc(double t) {
    if (t == 0.0) return 1.0;
    t = t * M_PI;
    return sin(t) / t;
}
__device__ static inline double fc_lanczos(double t) { return (-3.0 <= t && t < 3.0) ? fc_sinc(t) * fc_sinc(t / 3.0) : 0.0; }

// workspace (int32 words): windows [F][4] | bounds [F][2][side][2] = (xmin, n) | taps [F][2][side][kmax]
__global__ __launch_bounds__(256) void face_taps_kernel(int32_t* __restrict__ ws, int F, int side, int kmax) {
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= F * 2 * side) return;
    const int xx = id % side, axis = id / side % 2, f = id / (2 * side);
    const int32_t* win = ws + 4 * f;
    const int in_size = axis ? win[3] - win[1] : win[2] - win[0];
    int32_t* bounds = ws + 4 * (long)F + 2 * (long)id;
    int32_t* taps = ws + 4 * (long)F + 4 * (long)F * side + (long)id * kmax;
    if (in_size == side) {           // the skipped pass
        bounds[0] = xx, bounds[1] = 1;
        taps[0] = 1 << FC_BITS;
        for (int x = 1; x < kmax; ++x) taps[x] = 0;
        return;
    }
    const AxisGeom g = axis_geom(in_size, side);
    const double center = ((double)xx + 0.5) * g.scale;
    int xmin = (int)(center - g.support + 0.5);
    if (xmin < 0) xmin = 0;
    int n = (int)(center + g.support + 0.5);
    if (n > in_size) n = in_size;
    n -= xmin;
    if (n > kmax) n = kmax;          // cannot happen (n <= ksize <= kmax); keeps every store inside the row whatever the caller did
    if (n < 0) n = 0;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += fc_lanczos(((double)(x + xmin) - center + 0.5) / g.fs);
    for (int x = 0; x < n; ++x) {
        double w = fc_lanczos(((double)(x + xmin) - center + 0.5) / g.fs);      // the same bits as in the sum above
        if (ww != 0.0) w = w / ww;
        taps[x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << FC_BITS)) : (int)(0.5 + w * (double)(1 << FC_BITS));
    }
    for (int x = n; x < kmax; ++x) taps[x] = 0;
    bounds[0] = xmin, bounds[1] = n;
}

__device__ __forceinline__ uint8_t fc_clip8(int acc) {
    const int v = acc >> FC_BITS;    // arithmetic shift
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// grid (tiles, F), 256 threads.  LDS: `cap` rows of S * 3 bytes, rows [first, first + R) of the horizontally resampled crop.
__global__ __launch_bounds__(256) void face_crop_kernel(const uint8_t* __restrict__ frame, int H, int W, const int32_t* __restrict__ ws, int F,
                                                        int side, int kmax, int ox, int oy, int S, int tile, uint8_t* __restrict__ dst) {
    __shared__ uint8_t rows[FC_LDS_BYTES];
    const int f = blockIdx.y, y0 = blockIdx.x * tile, ny = min(tile, S - y0);
    const int left = ws[4 * f], top = ws[4 * f + 1];
    const int32_t* hb = ws + 4 * (long)F + 4 * (long)f * side;          // bounds of the horizontal axis, then of the vertical one
    const int32_t* vb = hb + 2 * side;
    const int32_t* ht = ws + 4 * (long)F + 4 * (long)F * side + 2 * (long)f * side * kmax;
    const int32_t* vt = ht + (long)side * kmax;
    const int pitch = S * 3, cap = FC_LDS_BYTES / pitch;
    const int first = vb[2 * (oy + y0)];
    const int last = vb[2 * (oy + y0 + ny - 1)] + vb[2 * (oy + y0 + ny - 1) + 1];     // xmin and xmin + n grow with the output index
    const int R = min(last - first, cap);            // the host chose `tile` so that last - first <= cap

    for (int it = threadIdx.x; it < R * S; it += 256) {
        const int r = it / S, x = it - r * S;
        const int fy = top + first + r;
        int a0 = 1 << (FC_BITS - 1), a1 = a0, a2 = a0;
        if (fy >= 0 && fy < H) {                     // rows of the crop outside the frame are 0
            const int xmin = hb[2 * (ox + x)], n = hb[2 * (ox + x) + 1];
            const int32_t* k = ht + (long)(ox + x) * kmax;
            const uint8_t* line = frame + (long)fy * W * 3;
            for (int t = 0; t < n; ++t) {
                const int fx = left + xmin + t;
                if (fx < 0 || fx >= W) continue;
                const uint8_t* p = line + (long)fx * 3;
                const int kt = k[t];
                a0 += kt * p[0], a1 += kt * p[1], a2 += kt * p[2];
            }
        }
        uint8_t* o = rows + r * pitch + x * 3;
        o[0] = fc_clip8(a0), o[1] = fc_clip8(a1), o[2] = fc_clip8(a2);
    }
    __syncthreads();

    uint8_t* out = dst + ((long)f * S + y0) * pitch;
    for (int it = threadIdx.x; it < ny * S; it += 256) {
        const int y = it / S, x = it - y * S;
        const int ymin = vb[2 * (oy + y0 + y)] - first, n = vb[2 * (oy + y0 + y) + 1];
        const int32_t* k = vt + (long)(oy + y0 + y) * kmax;
        int a0 = 1 << (FC_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n && ymin + t < R; ++t) {
            const uint8_t* p = rows + (ymin + t) * pitch + x * 3;
            const int kt = k[t];
            a0 += kt * p[0], a1 += kt * p[1], a2 += kt * p[2];
        }
        uint8_t* o = out + (long)it * 3;
        o[0] = fc_clip8(a0), o[1] = fc_clip8(a1), o[2] = fc_clip8(a2);
    }
}

// Argument checks shared by both entry points; kmax = the batch's largest tap bound, tile = output rows per workgroup such that
// the rows one workgroup keeps fit the LDS for every face.
static int face_crop_plan(const int32_t* windows, int F, int side, int S, int* kmax, int* tile) {
    FN_REQUIRE(windows && F > 0 && F <= 65535, "face_crop: F = %d windows (1 .. 65535 expected)", F);
    FN_REQUIRE(side > 0 && side <= FN_FACE_CROP_MAX_SIDE, "face_crop: side %d outside 1 .. %d", side, FN_FACE_CROP_MAX_SIDE);
    FN_REQUIRE(S > 0 && S <= side, "face_crop: output window of %d rows for side %d", S, side);
    const int cap = FC_LDS_BYTES / (S * 3);
    int km = 1, tl = FC_MAX_TILE;
    for (int f = 0; f < F; ++f) {
        const int32_t* w = windows + 4 * f;
        const long cw = (long)w[2] - w[0], ch = (long)w[3] - w[1];
        FN_REQUIRE(cw > 0 && ch > 0 && cw <= FN_FACE_CROP_MAX_EXTENT && ch <= FN_FACE_CROP_MAX_EXTENT,
                   "face_crop: window %d is %ld x %ld pixels (1 .. %d per axis expected)", f, cw, ch, FN_FACE_CROP_MAX_EXTENT);
        FN_REQUIRE(w[0] > -(1 << 24) && w[1] > -(1 << 24) && w[2] < (1 << 24) && w[3] < (1 << 24), "face_crop: window %d out of range", f);
        const AxisGeom gh = axis_geom((int)cw, side), gv = axis_geom((int)ch, side);
        km = gh.ksize > km ? gh.ksize : km;
        km = gv.ksize > km ? gv.ksize : km;
        // rows spanned by t output rows: at most (t - 1) * scale + 2 * support + 1 (section 17), t rows for a copied axis
        int t = FC_MAX_TILE;
        if ((int)ch != side)
            while (t > 1 && (double)(t - 1) * gv.scale + 2.0 * gv.support + 2.0 > (double)cap) --t;
        FN_REQUIRE((int)ch == side ? t <= cap : 2.0 * gv.support + 2.0 <= (double)cap, "face_crop: window %d does not fit the LDS plan", f);
        tl = t < tl ? t : tl;
    }
    *kmax = km, *tile = tl;
    return FN_OK;
}

static long long face_crop_words(int F, int side, int kmax) { return 4ll * F + 2ll * F * side * (2 + kmax); }

extern "C" int fn_face_crop_workspace(const int32_t* windows, int F, int side, long long* words) {
    int kmax = 0, tile = 0;
    FN_REQUIRE(words, "face_crop_workspace: bad arguments");
    const int rc = face_crop_plan(windows, F, side, side, &kmax, &tile);
    if (rc != FN_OK) return rc;
    *words = face_crop_words(F, side, kmax);
    return FN_OK;
}

extern "C" int fn_face_crop_resize_u8(const uint8_t* frame, int H, int W, const int32_t* windows, int F, int side, int ox, int oy, int S,
                                      uint8_t* dst, int32_t* workspace, long long workspace_words, void* stream) {
    FN_REQUIRE(frame && dst && workspace && H > 0 && W > 0 && (long)H * W * 3 < (1l << 40), "face_crop: bad arguments");
    int kmax = 0, tile = 0;
    const int rc = face_crop_plan(windows, F, side, S, &kmax, &tile);
    if (rc != FN_OK) return rc;
    FN_REQUIRE(ox >= 0 && oy >= 0 && ox + S <= side && oy + S <= side, "face_crop: output window (%d, %d) + %d exceeds side %d", ox, oy, S, side);
    FN_REQUIRE(workspace_words >= face_crop_words(F, side, kmax) && (long long)F * 2 * side * kmax < (1ll << 31),
               "face_crop: workspace of %lld words, %lld needed", workspace_words, face_crop_words(F, side, kmax));
    // Output rows per workgroup, within the LDS plan: a short tile filters its ~6 * scale + 1 halo rows again for few output
    // rows, a tall one leaves most of the 256 CUs idle when a photo has few faces.  About 512 workgroups per launch measured
    // best at 1, 8 and 32 faces (profiles/face_crop_bench.txt).
    const int want = cdiv((long)F * S, 512);
    if (want < tile) tile = want;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(workspace, windows, sizeof(int32_t) * 4 * F, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("face_crop: copying the windows to the device failed");
        return FN_ELAUNCH;
    }
    hipLaunchKernelGGL(face_taps_kernel, dim3(cdiv((long)F * 2 * side, 256)), dim3(256), 0, st, workspace, F, side, kmax);
    hipLaunchKernelGGL(face_crop_kernel, dim3(cdiv(S, tile), F), dim3(256), 0, st, frame, H, W, workspace, F, side, kmax, ox, oy, S, tile, dst);
    return check_launch("face_crop");
}

}  // namespace fn
