// Confidence maps of the soft-argmin's softmax (an addition beyond the reference's interface): per
// output pixel, from the bilinearly blended costs v_d of csrc/softargmin.hip (same coordinate rule, output size, zero-weight
// tap rule and fp32 weights as mvsgi_softargmin_scaled_f32),
//   m = max_d v_d, g_d = m - v_d, e_d = exp(-g_d), S = sum e_d, p_d = e_d / S, w_d = inv_idx[d], mu = (sum e_d w_d) / S
//   max_prob = max_d p_d                     = 1 / S                                (the winner's e is exactly 1)
//   entropy  = -sum p_d ln p_d               = ln S + (sum e_d g_d) / S             (every term >= 0: no cancellation; e_d == 0
//                                                                                    contributes 0, g_d = +inf included)
//   spread   = sqrt(sum p_d (w_d - mu)^2) / post_div = sqrt((sum e_d (w_d - mu)^2) / S) / post_div   (a second walk, mu known)
//   argmax   = the lowest d with v_d == m, -1 where the float maps are NaN
// One thread per output pixel, one launch, no [B, D, OH, OW] tensor anywhere: the low-resolution costs are read again (they
// are what the cost head just wrote).  D <= 16 and D <= 32 gather the blended candidates ONCE into registers; larger D walks
// them again per pass, as softargmin_pixel() does.  The blend is sa_blend() in every form and the file is compiled with
// -ffp-contract=off: the expression written here is the expression that runs, whichever maps are asked for.
// Non-finite costs as in the soft-argmin: a NaN or +inf cost under a non-zero weight, or every candidate -inf, makes S NaN
// and with it all three float maps (argmax -1); a single -inf candidate has e = 0 exactly.
#include "common.hpp"

#include <cmath>

namespace {

#include "softargmin_axes.hpp"

struct ConfSums {
    float S, T, G;
};

// e = exp(-g) into the sums; -> e
__device__ __forceinline__ float conf_accumulate(ConfSums& a, float m, float v, float w) {
    const float g = m - v;
    const float e = expf(-g);
    a.S = a.S + e;
    a.T = fmaf(e, w, a.T);
    if (e != 0.f) a.G = fmaf(e, g, a.G);
    return e;
}

__device__ __forceinline__ float conf_variance_term(float V, float e, float w, float mu) {
    const float dw = w - mu;
    return fmaf(e, dw * dw, V);
}

template <int DMAX>
__global__ __launch_bounds__(256) void confidence_kernel(const float* __restrict__ costs, const float* __restrict__ inv_idx,
                                                         float* __restrict__ max_prob, float* __restrict__ entropy,
                                                         float* __restrict__ spread, int* __restrict__ argmax,
                                                         int D, int H, int W, int OH, int OW, float rs, float post_div, float ln_d) {
    // grid = (ceil(OW / 256), OH, B)
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= OW) return;
    const int oy = blockIdx.y, b = blockIdx.z;
    const long long idx = ((long long)b * OH + oy) * OW + ox;
    const Axis2 ay = axis2f(oy, H, rs), ax = axis2f(ox, W, rs);
    const long long HW = (long long)H * W;
    const float* cb = costs + (long long)b * D * HW;
    const Taps taps = sa_taps(ay, ax, W);
    auto sample = [&](int d) { return sa_sample(cb + d * HW, ay, ax, taps); };

    float m = -INFINITY, V = 0.f, mu;
    int k = 0;
    ConfSums a = {0.f, 0.f, 0.f};
    if constexpr (DMAX > 0) {
        float v[DMAX];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            v[d] = d < D ? sample(d) : -INFINITY;
            if (v[d] > m) {                      // strict: the lowest index of a tie set
                m = v[d];
                k = d;
            }
        }
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
            if (d < D) v[d] = conf_accumulate(a, m, v[d], inv_idx[d]);
        mu = a.T / a.S;
        if (spread) {
#pragma unroll
            for (int d = 0; d < DMAX; ++d)
                if (d < D) V = conf_variance_term(V, v[d], inv_idx[d], mu);
        }
    } else {
        for (int d = 0; d < D; ++d) {
            const float v = sample(d);
            if (v > m) {
                m = v;
                k = d;
            }
        }
        for (int d = 0; d < D; ++d) conf_accumulate(a, m, sample(d), inv_idx[d]);
        mu = a.T / a.S;
        if (spread) {
            for (int d = 0; d < D; ++d) V = conf_variance_term(V, expf(-(m - sample(d))), inv_idx[d], mu);
        }
    }
    if (max_prob) max_prob[idx] = 1.0f / a.S;
    if (entropy) {
        const float h = logf(a.S) + a.G / a.S;
        entropy[idx] = ln_d != 0.f ? h / ln_d : h;
    }
    if (spread) {
        const float sd = sqrtf(V / a.S);
        spread[idx] = post_div == 1.0f ? sd : sd / post_div;
    }
    if (argmax) argmax[idx] = a.S != a.S ? -1 : k;
}

}  // namespace

extern "C" int mvsgi_confidence_f32(const float* costs, const float* inv_idx, float* max_prob, float* entropy, float* spread,
                                    int* argmax, int B, int D, int H, int W, double scale, int OH, int OW, float post_div,
                                    int normalize_entropy, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(costs && inv_idx, "mvsgi_confidence_f32: null pointer");
    MVSGI_REQUIRE(max_prob || entropy || spread || argmax, "mvsgi_confidence_f32: all four outputs are null");
    MVSGI_REQUIRE(post_div != 0.0f, "mvsgi_confidence_f32: post_div must be non-zero");
    MVSGI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mvsgi_confidence_f32: non-positive dimension");
    MVSGI_REQUIRE(std::isfinite(scale) && scale > 0.0, "mvsgi_confidence_f32: scale %g is not a finite positive factor", scale);
    // F.interpolate: floor(in * scale) in double
    const double oh = std::floor((double)H * scale), ow = std::floor((double)W * scale);
    MVSGI_REQUIRE(oh >= 1.0 && ow >= 1.0, "mvsgi_confidence_f32: scale %g gives an empty %g x %g output for %d x %d", scale, oh, ow, H, W);
    MVSGI_REQUIRE(oh < 65536.0 && ow < 2147483648.0 && B < 65536,
                  "mvsgi_confidence_f32: output %g x %g (B = %d) exceeds the launch geometry", oh, ow, B);
    MVSGI_REQUIRE(OH == (int)oh && OW == (int)ow, "mvsgi_confidence_f32: caller's output %d x %d is not floor(%d x %d * %g) = %d x %d",
                  OH, OW, H, W, scale, (int)oh, (int)ow);
    const float rs = (float)(1.0 / scale);
    const float ln_d = (normalize_entropy && D > 1) ? (float)std::log((double)D) : 0.f;      // D == 1: the entropy is 0 as it is
    auto kern = D <= 16 ? confidence_kernel<16> : (D <= 32 ? confidence_kernel<32> : confidence_kernel<0>);
    hipLaunchKernelGGL(kern, dim3((unsigned)mvsgi::cdiv(OW, 256), (unsigned)OH, (unsigned)B), dim3(256), 0, mvsgi::as_stream(stream),
                       costs, inv_idx, max_prob, entropy, spread, argmax, D, H, W, OH, OW, rs, post_div, ln_d);
    return mvsgi::check_launch("mvsgi_confidence_f32");
}
