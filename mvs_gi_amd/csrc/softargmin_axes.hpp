// The coordinate rule, the taps of a pixel and the blend that csrc/softargmin.hip (upsample + softmax + expectation),
// csrc/confidence.hip (the confidence maps of the same softmax) and csrc/losses.hip (the cross-entropy on it) share: one
// definition, so that all of them blend the same value of a candidate at a pixel.
// Include inside the translation unit's anonymous namespace (behind common.hpp), as device_prims.hpp is.
#pragma once

struct Axis2 {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Axis2 axis2(int dst, int in, int scale) {
    Axis2 a;
    if (scale == 1) {
        a.i0 = a.i1 = dst;
        a.l0 = 1.f;
        a.l1 = 0.f;
        return a;
    }
    // F.interpolate(scale_factor=s) uses 1/s as the coordinate scale
    float src = ((float)dst + 0.5f) * (1.0f / (float)scale) - 0.5f;
    src = src < 0.f ? 0.f : src;
    a.i0 = (int)src;
    if (a.i0 > in - 1) a.i0 = in - 1;
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

// The blend of the multi-pass forms (D > 32 per pixel, DMAX = 0 per row pair / band), which compute it once per pass (max,
// sums, norm_costs).  Left to the compiler, each pass is contracted on its own (the scalar tail stores of norm_costs fused the
// outer sum where the two passes before did not), and norm_costs were quotients of other exponentials than the sum holds:
// the winner's exp(v' - m) was exp(-ulp(v)) instead of 1 -- 2e-3 low at |cost| ~ 3e4 -- and sum_d p_d missed 1 by the blend's
// rounding (4e-6 at |cost| ~ 40) instead of the sum's (D + 2) 2^-24.  Every rounding is fixed here: all passes see one value.
__device__ __forceinline__ float sa_blend(float ly0, float ly1, float lx0, float lx1, float a0, float a1, float b0, float b1) {
    return fmaf(ly1, fmaf(lx1, b1, lx0 * b0), ly0 * fmaf(lx1, a1, lx0 * a0));
}

// ATen's rule for F.interpolate(scale_factor = s, mode = 'bilinear', align_corners = False, recompute_scale_factor = None):
// source coordinate max((dst + 0.5) * rs - 0.5, 0) with rs = 1 / s rounded to fp32 once on the host.  axis2() above is this
// for s = 1 | 2.
__device__ __forceinline__ Axis2 axis2f(int dst, int in, float rs) {
    Axis2 a;
    float src = ((float)dst + 0.5f) * rs - 0.5f;
    src = src < 0.f ? 0.f : src;
    a.i0 = (int)src;
    if (a.i0 > in - 1) a.i0 = in - 1;
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

// The taps of an output pixel inside a candidate's [H][W] plane.  A tap under a weight of exactly 0 is not blended: it enters the
// expression as 0, whatever it holds.  Every pixel at scale 1 and the centre-aligned pixels of an odd factor have such a tap
// (l1 == 0, i1 = i0 + 1), and 0 * c would turn a -inf or NaN cost of the NEIGHBOURING pixel into a NaN here.  Finite costs give
// the same bits either way (0 * c = 0 * 0).
struct Taps {
    long long o00, o01, o10, o11;
    bool x1, y1;                                 // the right column's / the lower row's weight is 0
};

__device__ __forceinline__ Taps sa_taps(const Axis2& ay, const Axis2& ax, int W) {
    Taps t;
    t.o00 = (long long)ay.i0 * W + ax.i0, t.o01 = (long long)ay.i0 * W + ax.i1;
    t.o10 = (long long)ay.i1 * W + ax.i0, t.o11 = (long long)ay.i1 * W + ax.i1;
    t.x1 = ax.l1 == 0.f, t.y1 = ay.l1 == 0.f;
    return t;
}

struct TapValues {
    float p00, p01, p10, p11;
};

// the four taps of the candidate whose plane is p
__device__ __forceinline__ TapValues sa_fetch(const float* p, const Taps& t) {
    TapValues v;
    v.p01 = t.x1 ? 0.f : p[t.o01], v.p10 = t.y1 ? 0.f : p[t.o10], v.p11 = (t.x1 || t.y1) ? 0.f : p[t.o11];
    v.p00 = p[t.o00];
    return v;
}

// the candidate's value at the pixel, by sa_blend
__device__ __forceinline__ float sa_sample(const float* p, const Axis2& ay, const Axis2& ax, const Taps& t) {
    const TapValues v = sa_fetch(p, t);
    return sa_blend(ay.l0, ay.l1, ax.l0, ax.l1, v.p00, v.p01, v.p10, v.p11);
}
