// The reference's bilinear_grid_sample (dsta_mvs/model/backports/backports.py:34-86, align_corners=False, zero padding), once:
// the tap set-up and the fetches that K1 (sweep.hip), the fisheye resampler (resample.hip) and the back-projection
// (reproject.hip) evaluate operation by operation with fp contraction off -- one text, so the three agree by construction --
// and what the resampler and the back-projection share around their four-pixel sampling stage: the image kinds, the / 255
// table and its staging, the host's tap-offset check and the kind x vector dispatch.
// Include inside the translation unit's anonymous namespace, after common.hpp.
#pragma once

#include "device_prims.hpp"

struct Bilin {
    int o00, o01, o10, o11;     // pixel offsets y*W+x, or -1 when the tap is outside
    float w00, w01, w10, w11;   // weights of (x0,y0), (x0,y1), (x1,y0), (x1,y1)
};

__device__ __forceinline__ Bilin bilin_setup(float gx, float gy, int W, int H) {
#pragma clang fp contract(off)
    Bilin t;
    // backports.py:41-42 (align_corners=False)
    const float x = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
    const float y = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    const float xf = floorf(x), yf = floorf(y);
    const float x1f = xf + 1.0f, y1f = yf + 1.0f;
    // backports.py:52-55: weights from the unclamped coordinates
    t.w00 = (x1f - x) * (y1f - y);
    t.w01 = (x1f - x) * (y - yf);
    t.w10 = (x - xf) * (y1f - y);
    t.w11 = (x - xf) * (y - yf);
    // anything further out than one texel is outside anyway; clamping first keeps the
    // float->int conversion defined for huge or NaN coordinates
    const int x0 = (int)fminf(fmaxf(xf, -2.0f), (float)W + 1.0f);
    const int y0 = (int)fminf(fmaxf(yf, -2.0f), (float)H + 1.0f);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = (x0 >= 0) & (x0 < W), vx1 = (x1 >= 0) & (x1 < W);
    const bool vy0 = (y0 >= 0) & (y0 < H), vy1 = (y1 >= 0) & (y1 < H);
    t.o00 = (vx0 & vy0) ? y0 * W + x0 : -1;
    t.o01 = (vx0 & vy1) ? y1 * W + x0 : -1;
    t.o10 = (vx1 & vy0) ? y0 * W + x1 : -1;
    t.o11 = (vx1 & vy1) ? y1 * W + x1 : -1;
    return t;
}

// the four taps of a fp32 plane
__device__ __forceinline__ float bilin_fetch(const float* __restrict__ plane, const Bilin& t) {
#pragma clang fp contract(off)
    // zero padding: a tap outside the image reads 0 (backports.py:58-72)
    const float i00 = t.o00 >= 0 ? plane[t.o00] : 0.0f;
    const float i01 = t.o01 >= 0 ? plane[t.o01] : 0.0f;
    const float i10 = t.o10 >= 0 ? plane[t.o10] : 0.0f;
    const float i11 = t.o11 >= 0 ? plane[t.o11] : 0.0f;
    // backports.py:86: Ia*wa + Ib*wb + Ic*wc + Id*wd, left to right
    return ((i00 * t.w00 + i01 * t.w01) + i10 * t.w10) + i11 * t.w11;
}

// the same for channel c of an interleaved uint8 RGB image; lut[k] = RN(k / 255.0f)
__device__ __forceinline__ float bilin_fetch_u8(const unsigned char* __restrict__ img, int c, const float* lut, const Bilin& t) {
#pragma clang fp contract(off)
    const float i00 = t.o00 >= 0 ? lut[img[t.o00 * 3 + c]] : 0.0f;
    const float i01 = t.o01 >= 0 ? lut[img[t.o01 * 3 + c]] : 0.0f;
    const float i10 = t.o10 >= 0 ? lut[img[t.o10 * 3 + c]] : 0.0f;
    const float i11 = t.o11 >= 0 ? lut[img[t.o11 * 3 + c]] : 0.0f;
    return ((i00 * t.w00 + i01 * t.w01) + i10 * t.w10) + i11 * t.w11;
}

// RN(k / 255.0f), k = 0..255, evaluated by the host compiler (IEEE single division): a uint8 image is converted as the
// facade does (api/inference_pytorch.py:58-59: .float() / 255.0)
struct U8Table {
    float v[256];
};
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
    return t;
}

// ---- What surrounds the four-pixel sampling stage of resample_bilinear_kernel and reproject_kernel (blocks of 256 threads).
// The stage itself stays written out in both kernels: as a shared function it moves resample_bilinear_kernel's code.

// layout of the images a kernel samples (the numeric values are the C ABI's image kinds), or no images at all
enum ImageKind { U8HWC3 = 0, F32CHW = 1, NO_IMAGES = 2 };

__constant__ U8Table kU8Dev = make_u8_table();

// the / 255 table into the block's LDS (lut: __shared__ float[256]); every thread of the block calls it
template <int IN>
__device__ __forceinline__ void stage_u8_table(float* lut) {
    if (IN == U8HWC3) {
        lut[threadIdx.x] = kU8Dev.v[threadIdx.x];
        __syncthreads();
    }
}

// tap offsets are 32-bit: (y * Wr + x) * 3 + c for the interleaved bytes, y * Wr + x within a fp32 plane, y up to Hr + 1
inline int check_tap_offsets(const char* what, const char* noun, int in, int Hr, int Wr) {
    const long long row_bytes = (long long)Wr * (in == U8HWC3 ? 3 : 4);
    MVSGI_REQUIRE(row_bytes < (1ll << 23) && ((long long)Hr + 2) * row_bytes < (1ll << 31),
                  "%s: %s %d x %d: row bytes %lld (limit 2^23) or image bytes beyond the 32-bit tap offsets", what, noun, Hr, Wr,
                  row_bytes);
    return 0;
}

// LAUNCH(IN, VEC) for the image kind `in` (U8HWC3 or F32CHW) and vec = W % 4 == 0
#define MVSGI_LAUNCH_IMAGE_KIND_VEC(LAUNCH, in, vec)                             \
    do {                                                                         \
        if ((in) == U8HWC3) {                                                    \
            if (vec) LAUNCH(U8HWC3, true); else LAUNCH(U8HWC3, false);           \
        } else {                                                                 \
            if (vec) LAUNCH(F32CHW, true); else LAUNCH(F32CHW, false);           \
        }                                                                        \
    } while (0)
