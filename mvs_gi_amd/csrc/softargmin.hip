// K4: fused bilinear upsample + softmax over D + expectation, fp32.
// Replaces DistanceRegressorWithFixedCandidates.forward
// (dsta_mvs/model/distance_regressor/distance_regressor.py:51-79):
//   c = costs[:, 0]; c = interpolate(c, scale_factor=s, bilinear); p = softmax(c, 1);
//   inv_dist = sum_d p_d * inv_idx_d.
// One thread per output pixel.  For D <= 32 the D blended samples are gathered ONCE into
// registers (4 taps each) and max / exp / sums / probabilities are computed from them (the
// first version walked the candidates three times: 192 instead of 64 loads and 32 instead of
// 16 exps per pixel at D = 16); larger D keeps the multi-pass walk.  The upsampled
// [B, D, sH, sW] volume and the probabilities never touch HBM unless the caller asks for
// norm_costs (training only; inference discards it, spherical_sweep_stereo.py:266).  The 4 source pixels of neighbouring lanes coincide or
// are adjacent, so every candidate plane is read once from HBM and served from L1/L2 after.
#include "common.hpp"

#include <cmath>
#include <cstdlib>

namespace {

#include "device_prims.hpp"

#include "softargmin_axes.hpp"

// One output pixel of either thread-per-pixel kernel; axis(dst, in) is the coordinate rule (axis2 | axis2f).
template <class Axis>
__device__ __forceinline__ void softargmin_pixel(const float* __restrict__ costs, const float* __restrict__ inv_idx,
                                                 float* __restrict__ inv_dist, float* __restrict__ norm_costs,
                                                 int D, int H, int W, int OH, int OW, int ox, float post_div, Axis axis) {
    const int oy = blockIdx.y, b = blockIdx.z;
    const long long idx = ((long long)b * OH + oy) * OW + ox;
    const Axis2 ay = axis(oy, H), ax = axis(ox, W);
    const long long HW = (long long)H * W;
    const float* cb = costs + (long long)b * D * HW;
    const Taps taps = sa_taps(ay, ax, W);
    // this file is compiled with contraction on: the expression below, as the compiler contracts it, is what defines the bits
    auto sample = [&](int d) {
        const TapValues v = sa_fetch(cb + d * HW, taps);
        return ay.l0 * (ax.l0 * v.p00 + ax.l1 * v.p01) + ay.l1 * (ax.l0 * v.p10 + ax.l1 * v.p11);
    };

    if (D <= 32) {
        float v[32];
        float m = -INFINITY;
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            v[d] = d < D ? sample(d) : -INFINITY;
            m = fmaxf(m, v[d]);
        }
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            if (d < D) {
                v[d] = expf(v[d] - m);
                s += v[d];
                t = fmaf(v[d], inv_idx[d], t);
            }
        }
        const float r = t / s;
        inv_dist[idx] = post_div == 1.0f ? r : r / post_div;
        if (norm_costs) {
            const long long OHW = (long long)OH * OW;
            float* np = norm_costs + (long long)b * D * OHW + (long long)oy * OW + ox;
            const float rs = 1.0f / s;
#pragma unroll
            for (int d = 0; d < 32; ++d)
                if (d < D) np[d * OHW] = v[d] * rs;
        }
        return;
    }
    // the same taps; one rounding order for all three passes, see sa_blend()
    auto sample_mp = [&](int d) { return sa_sample(cb + d * HW, ay, ax, taps); };
    float m = -INFINITY;
    for (int d = 0; d < D; ++d) m = fmaxf(m, sample_mp(d));
    float s = 0.f, t = 0.f;
    for (int d = 0; d < D; ++d) {
        const float e = expf(sample_mp(d) - m);
        s += e;
        t = fmaf(e, inv_idx[d], t);
    }
    const float r = t / s;
    inv_dist[idx] = post_div == 1.0f ? r : r / post_div;
    if (norm_costs) {
        const long long OHW = (long long)OH * OW;
        float* np = norm_costs + (long long)b * D * OHW + (long long)oy * OW + ox;
        for (int d = 0; d < D; ++d) np[d * OHW] = expf(sample_mp(d) - m) / s;
    }
}


__global__ __launch_bounds__(256) void softargmin_kernel(const float* __restrict__ costs,
                                                         const float* __restrict__ inv_idx,
                                                         float* __restrict__ inv_dist, float* __restrict__ norm_costs,
                                                         int B, int D, int H, int W, int scale, float post_div) {
    // grid = (ceil(OW / 256), OH, B)
    const int OH = H * scale, OW = W * scale;
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= OW) return;
    softargmin_pixel(costs, inv_idx, inv_dist, norm_costs, D, H, W, OH, OW, ox, post_div,
                     [scale](int dst, int in) { return axis2(dst, in, scale); });
}

// ---------------------------------------------------------------------------------------------
// scale == 2: one workgroup per (frame, low-resolution row pair k | k + 1, column tile).  Output rows 2k + 1 and 2k + 2 blend
// exactly those two rows, so the workgroup stages them for all D candidates in LDS ONCE (16-byte loads; the thread-per-pixel
// kernel above fetched every cost row pair from beyond L2 five times, PMC: 544 MB for a 105 MB input) and each thread
// finishes FOUR consecutive output pixels of one row: the four low-resolution columns c0 - 1 .. c0 + 2 they blend come from
// three LDS reads per row and candidate, and inv_dist / norm_costs leave as 16-byte stores (1 KiB per wave instruction instead
// of 256 B).  The arithmetic of a pixel is the expression of the kernel above, term for term (same taps, same weights: the
// clamped edge taps are staged replicated, where they carry the weights axis2() gives them).
// Logical unit order (b, k, x-tile) walks XCD-contiguously: the unit of row pair k + 1 finds row k + 1 in its XCD's L2.
// DMAX = 16 | 32: the blended candidates of the four pixels live in registers; DMAX = 0: any D, three passes over LDS.
// ---------------------------------------------------------------------------------------------

template <int DMAX>
__global__ __launch_bounds__(DMAX == 32 ? 512 : 640) void softargmin_rows_kernel(const float* __restrict__ costs, const float* __restrict__ inv_idx,
                                                               float* __restrict__ inv_dist, float* __restrict__ norm_costs,
                                                               int B, int D, int H, int W, int xt, int xtiles, int units,
                                                               float post_div, int contiguous) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int u = contiguous ? xcd_remap((int)blockIdx.x, units) : (int)blockIdx.x;
    const int xtile = u % xtiles;
    int tq = u / xtiles;
    const int k = tq % (H + 1) - 1;
    const int b = tq / (H + 1);
    const int x0 = xtile * xt;
    const int r0 = k < 0 ? 0 : k, r1 = k + 1 > H - 1 ? H - 1 : k + 1;
    const int Wp = xt + 4;                       // LDS row: index i holds column x0 + i - 2 (clamped to the image)
    const long long HW = (long long)H * W;
    const float* cb = costs + (long long)b * D * HW;
    const int xv = W - x0 < xt ? W - x0 : xt;    // columns of this tile inside the image

    // ---- stage rows r0, r1 of every candidate: LDS[(row * D + d) * Wp + i] ----
    const int nrow = 2 * D;
    if ((W & 3) == 0 && (xt & 3) == 0) {         // x0, xv multiples of 4: 16-byte loads, two 8-byte LDS stores
        const int nq = xv >> 2;
        for (int e = tid; e < nrow * nq; e += nthr) {
            const int p = e / nq, q = e - p * nq;
            const int row = p >= D, d = p - row * D;
            const f32x4 v = *reinterpret_cast<const f32x4*>(cb + d * HW + (long long)(row ? r1 : r0) * W + x0 + 4 * q);
            float* dst = sa_lds + p * Wp + 4 * q + 2;
            *reinterpret_cast<f32x2*>(dst) = f32x2{v[0], v[1]};
            *reinterpret_cast<f32x2*>(dst + 2) = f32x2{v[2], v[3]};
        }
    } else {
        for (int e = tid; e < nrow * xv; e += nthr) {
            const int p = e / xv, c = e - p * xv;
            const int row = p >= D, d = p - row * D;
            sa_lds[p * Wp + c + 2] = cb[d * HW + (long long)(row ? r1 : r0) * W + x0 + c];
        }
    }
    {   // the halo: column x0 - 1 (index 1) and columns x0 + xv .. x0 + xt (indices xv + 2 .. xt + 2), clamped = replicated
        const int npad = 2 + xt - xv;
        for (int e = tid; e < nrow * npad; e += nthr) {
            const int p = e / npad, h = e - p * npad;
            const int row = p >= D, d = p - row * D;
            const int i = h == 0 ? 1 : xv + 1 + h;
            int c = x0 + i - 2;
            c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
            sa_lds[p * Wp + i] = cb[d * HW + (long long)(row ? r1 : r0) * W + c];
        }
    }
    __syncthreads();

    const int half = xt >> 1;                    // threads per output row
    const int rr = tid >= half, j = tid - rr * half;
    const int oy = 2 * k + 1 + rr, c0 = x0 + 2 * j;
    const int OH = 2 * H, OW = 2 * W;
    if (tid >= 2 * half || oy < 0 || oy >= OH || c0 >= W) return;
    const Axis2 ay = axis2(oy, H, 2);
    float l0[4], l1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ox = 2 * c0 + e;
        const Axis2 ax = axis2(ox < OW ? ox : OW - 1, W, 2);
        l0[e] = ax.l0;
        l1[e] = ax.l1;
    }
    const float* la = sa_lds + 2 * j + 1;        // q0 = column c0 - 1
    const float* lb = la + D * Wp;
    // taps of output pixel e: (q0, q1), (q1, q2), (q1, q2), (q2, q3)
    auto blend4 = [&](int d, float (&o)[4]) {
        const float* pa = la + d * Wp;
        const float* pb = lb + d * Wp;
        const float a0 = pa[0], a3 = pa[3], b0 = pb[0], b3 = pb[3];
        const f32x2 am = *reinterpret_cast<const f32x2*>(pa + 1), bm = *reinterpret_cast<const f32x2*>(pb + 1);
        const float at0[4] = {a0, am[0], am[0], am[1]}, at1[4] = {am[0], am[1], am[1], a3};
        const float bt0[4] = {b0, bm[0], bm[0], bm[1]}, bt1[4] = {bm[0], bm[1], bm[1], b3};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (DMAX == 0)             // blended again in every pass: the roundings are spelled out, see sa_blend()
                o[e] = sa_blend(ay.l0, ay.l1, l0[e], l1[e], at0[e], at1[e], bt0[e], bt1[e]);
            else
                o[e] = ay.l0 * (l0[e] * at0[e] + l1[e] * at1[e]) + ay.l1 * (l0[e] * bt0[e] + l1[e] * bt1[e]);
        }
    };
    const long long OHW = (long long)OH * OW;
    const long long idx = ((long long)b * OH + oy) * OW + 2 * c0;
    const int nvalid = OW - 2 * c0 < 4 ? OW - 2 * c0 : 4;
    const bool vec = (OW & 3) == 0 && nvalid == 4;
    float* np = norm_costs ? norm_costs + (long long)b * D * OHW + (long long)oy * OW + 2 * c0 : nullptr;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};

    if constexpr (DMAX > 0) {
        float v[DMAX][4];
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            if (d < D) {
                blend4(d, v[d]);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[d][e]);
            }
        }
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            if (d < D) {
                const float w = inv_idx[d];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[d][e] = expf(v[d][e] - m[e]);
                    s[e] += v[d][e];
                    t[e] = fmaf(v[d][e], w, t[e]);
                }
            }
        }
        if (np) {
            float rs[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) rs[e] = 1.0f / s[e];
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                if (d < D) {
                    if (vec) {
                        // norm_costs leaves with nt stores (435 MB per 64 frames nothing on the path reads back): 164 -> 157 us
                        __builtin_nontemporal_store(f32x4{v[d][0] * rs[0], v[d][1] * rs[1], v[d][2] * rs[2], v[d][3] * rs[3]}, reinterpret_cast<f32x4*>(np + d * OHW));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (e < nvalid) np[d * OHW + e] = v[d][e] * rs[e];
                    }
                }
            }
        }
    } else {
        float o[4];
        for (int d = 0; d < D; ++d) {
            blend4(d, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], o[e]);
        }
        for (int d = 0; d < D; ++d) {
            blend4(d, o);
            const float w = inv_idx[d];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ex = expf(o[e] - m[e]);
                s[e] += ex;
                t[e] = fmaf(ex, w, t[e]);
            }
        }
        if (np) {
            for (int d = 0; d < D; ++d) {
                blend4(d, o);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nvalid) np[d * OHW + e] = expf(o[e] - m[e]) / s[e];
            }
        }
    }
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = t[e] / s[e];
        r[e] = post_div == 1.0f ? r[e] : r[e] / post_div;
    }
    if (vec) {
        *reinterpret_cast<f32x4*>(inv_dist + idx) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nvalid) inv_dist[idx + e] = r[e];
    }
}

// ---------------------------------------------------------------------------------------------
// Any other scale factor (mvsgi_softargmin_scaled_f32).  The coordinate rule is ATen's for F.interpolate(scale_factor = s,
// mode = 'bilinear', align_corners = False, recompute_scale_factor = None): output size floor(in * s), source coordinate
// max((dst + 0.5) * rs - 0.5, 0) with rs = 1 / s rounded to fp32 once on the host.  axis2() above is this for s = 1 | 2.
// ---------------------------------------------------------------------------------------------
// One thread per output pixel at any factor (fractional, down-scaling): softargmin_kernel with the float coordinate scale.
// It is the correctness path; integer factors >= 3 take the row-band kernel below.
__global__ __launch_bounds__(256) void softargmin_scaled_kernel(const float* __restrict__ costs, const float* __restrict__ inv_idx,
                                                                float* __restrict__ inv_dist, float* __restrict__ norm_costs,
                                                                int B, int D, int H, int W, int OH, int OW, float rs, float post_div) {
    // grid = (ceil(OW / 256), OH, B)
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= OW) return;
    softargmin_pixel(costs, inv_idx, inv_dist, norm_costs, D, H, W, OH, OW, ox, post_div,
                     [rs](int dst, int in) { return axis2f(dst, in, rs); });
}

// ---------------------------------------------------------------------------------------------
// Integer scale S >= 3: the row-pair kernel's unit, widened to a row band.  Unit (b, k, x-tile), k = -1 .. H - 1, stages
// low-resolution rows max(k, 0) and min(k + 1, H - 1) of all D candidates for xt columns exactly as softargmin_rows_kernel
// does (same LDS image: index i of a row holds column x0 + i - 2, clamped to the image) and finishes the S output rows
// S * k + S / 2 .. S * k + S / 2 + S - 1 that blend them (k = -1: the S / 2 rows above the first centre, k = H - 1: the
// (S + 1) / 2 rows below the last).  A work item is four consecutive output pixels of one row; the 256 threads walk the
// S * (S * xt / 4) items of the unit row by row, so a wave's 64 items are consecutive runs of one output row: lane l reads
// LDS column base + floor(4 l / S), which is conflict-free for S >= 4 (32 lanes touch at most 32 consecutive dwords, and
// lanes that share a column read one address: a broadcast) and 2-way on 8 of the 32 banks for S = 3 (32 runs span 43 columns).
// Four consecutive pixels blend at most three low-resolution columns for S >= 3: three LDS reads per row and candidate,
// the taps are selected from them by the offsets axis2f() gave (computed once per item, with the horizontal weights);
// X4 (S == 4, the full-resolution case) knows the taps at compile time and has no selects.
// The arithmetic of a pixel is softargmin_scaled_kernel's expression term for term, taps and weights from the same axis2f().
// (including its rule that a tap under a weight of exactly 0 -- the right / lower tap of a centre-aligned pixel of an odd S --
// is not blended; X4 and the x2 kernel have such taps only at the clamped image border and blend them as before).
// DMAX as above.
// ---------------------------------------------------------------------------------------------
template <int DMAX, bool X4>
__global__ __launch_bounds__(256) void softargmin_band_kernel(const float* __restrict__ costs, const float* __restrict__ inv_idx,
                                                              float* __restrict__ inv_dist, float* __restrict__ norm_costs,
                                                              int B, int D, int H, int W, int S, float rs, int xt, int xtiles, int units,
                                                              float post_div) {
    extern __shared__ __attribute__((aligned(16))) float sa_lds[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int u = xcd_remap((int)blockIdx.x, units);
    const int xtile = u % xtiles;
    const int tq = u / xtiles;
    const int k = tq % (H + 1) - 1;
    const int b = tq / (H + 1);
    const int x0 = xtile * xt;
    const int r0 = k < 0 ? 0 : k, r1 = k + 1 > H - 1 ? H - 1 : k + 1;
    const int Wp = xt + 4;
    const long long HW = (long long)H * W;
    const float* cb = costs + (long long)b * D * HW;
    const int xv = W - x0 < xt ? W - x0 : xt;    // columns of this tile inside the image

    // ---- stage rows r0, r1 of every candidate: LDS[(row * D + d) * Wp + i] ----
    const int nrow = 2 * D;
    if ((W & 3) == 0) {                          // x0, xv multiples of 4 (xt always is): 16-byte loads, two 8-byte LDS stores
        const int nq = xv >> 2;
        for (int e = tid; e < nrow * nq; e += nthr) {
            const int p = e / nq, q = e - p * nq;
            const int row = p >= D, d = p - row * D;
            const f32x4 v = *reinterpret_cast<const f32x4*>(cb + d * HW + (long long)(row ? r1 : r0) * W + x0 + 4 * q);
            float* dst = sa_lds + p * Wp + 4 * q + 2;
            *reinterpret_cast<f32x2*>(dst) = f32x2{v[0], v[1]};
            *reinterpret_cast<f32x2*>(dst + 2) = f32x2{v[2], v[3]};
        }
    } else {
        for (int e = tid; e < nrow * xv; e += nthr) {
            const int p = e / xv, c = e - p * xv;
            const int row = p >= D, d = p - row * D;
            sa_lds[p * Wp + c + 2] = cb[d * HW + (long long)(row ? r1 : r0) * W + x0 + c];
        }
    }
    {   // the halo: column x0 - 1 (index 1) and columns x0 + xv .. x0 + xt + 1 (indices xv + 2 .. xt + 3), clamped = replicated
        const int npad = 3 + xt - xv;
        for (int e = tid; e < nrow * npad; e += nthr) {
            const int p = e / npad, h = e - p * npad;
            const int row = p >= D, d = p - row * D;
            const int i = h == 0 ? 1 : xv + 1 + h;
            int c = x0 + i - 2;
            c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
            sa_lds[p * Wp + i] = cb[d * HW + (long long)(row ? r1 : r0) * W + c];
        }
    }
    __syncthreads();

    const int OH = S * H, OW = S * W;
    const long long OHW = (long long)OH * OW;
    const int runs = (S * xt) >> 2;              // items per output row of the tile (S * x0 and S * xt are multiples of 4)
    for (int it = tid; it < S * runs; it += nthr) {
        const int rr = it / runs, j = it - rr * runs;
        const int oy = S * k + (S >> 1) + rr, ox0 = S * x0 + 4 * j;
        if (oy < 0 || oy >= OH || ox0 >= OW) continue;
        const Axis2 ay = axis2f(oy, H, rs);
        float l0[4], l1[4];
        int s0[4], s1[4];                        // tap columns relative to the first pixel's left tap: s0 in {0, 1}, s1 in {0, 1, 2}
        int cbase = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ox = ox0 + e;
            const Axis2 ax = axis2f(ox < OW ? ox : OW - 1, W, rs);
            l0[e] = ax.l0;
            l1[e] = ax.l1;
            if constexpr (X4) {                  // S == 4: the run is the four phases of low-resolution column c = ox0 / 4
                s0[e] = e >> 1;                  // taps (c - 1, c), (c - 1, c), (c, c + 1), (c, c + 1), known at compile time: no
                s1[e] = (e >> 1) + 1;            // selects.  At the image border the clamped tap is the replicated halo column,
            } else {                             // under the weight axis2f() gave it, as in the row-pair kernel
                if (e == 0) cbase = ax.i0;
                s0[e] = ax.i0 - cbase;
                s1[e] = ax.i1 - cbase;
            }
        }
        if constexpr (X4) cbase = (ox0 >> 2) - 1;
        // ay.i0 == r0 by construction of the band.  For odd S whose fp32 reciprocal rounds below 1 / S the first row of a band
        // (source coordinate exactly k) can land an ulp under k with weight ~1 on row k: both taps then take row r0.
        const float* la = sa_lds + (cbase - x0 + 2);
        const float* lb = la + (ay.i0 == r0 ? D * Wp : 0);
        auto blend4 = [&](int d, float (&o)[4]) {
            const float* pa = la + d * Wp;
            const float* pb = lb + d * Wp;
            const float a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float at0 = s0[e] ? a1 : a0, at1 = s1[e] == 0 ? a0 : (s1[e] == 1 ? a1 : a2);
                const float bt0 = s0[e] ? b1 : b0, bt1 = s1[e] == 0 ? b0 : (s1[e] == 1 ? b1 : b2);
                if constexpr (X4) {              // no weight of an interior tap is 0 at S = 4 (phases 1/8, 3/8, 5/8, 7/8)
                    if constexpr (DMAX == 0)     // blended again in every pass: the roundings are spelled out, see sa_blend()
                        o[e] = sa_blend(ay.l0, ay.l1, l0[e], l1[e], at0, at1, bt0, bt1);
                    else
                        o[e] = ay.l0 * (l0[e] * at0 + l1[e] * at1) + ay.l1 * (l0[e] * bt0 + l1[e] * bt1);
                } else {                         // a tap under a weight of exactly 0 enters as 0, as in softargmin_pixel()
                    const float at1z = l1[e] == 0.f ? 0.f : at1, bt0z = ay.l1 == 0.f ? 0.f : bt0;
                    const float bt1z = (l1[e] == 0.f || ay.l1 == 0.f) ? 0.f : bt1;
                    if constexpr (DMAX == 0)
                        o[e] = sa_blend(ay.l0, ay.l1, l0[e], l1[e], at0, at1z, bt0z, bt1z);
                    else
                        o[e] = ay.l0 * (l0[e] * at0 + l1[e] * at1z) + ay.l1 * (l0[e] * bt0z + l1[e] * bt1z);
                }
            }
        };
        const long long idx = ((long long)b * OH + oy) * OW + ox0;
        const int nvalid = OW - ox0 < 4 ? OW - ox0 : 4;
        const bool vec = (OW & 3) == 0;          // then ox0 < OW has all four pixels inside and idx is 16-byte aligned
        float* np = norm_costs ? norm_costs + (long long)b * D * OHW + (long long)oy * OW + ox0 : nullptr;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};

        if constexpr (DMAX > 0) {
            float v[DMAX][4];
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                if (d < D) {
                    blend4(d, v[d]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[d][e]);
                }
            }
#pragma unroll
            for (int d = 0; d < DMAX; ++d) {
                if (d < D) {
                    const float w = inv_idx[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[d][e] = expf(v[d][e] - m[e]);
                        s[e] += v[d][e];
                        t[e] = fmaf(v[d][e], w, t[e]);
                    }
                }
            }
            if (np) {
                float rcp[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) rcp[e] = 1.0f / s[e];
#pragma unroll
                for (int d = 0; d < DMAX; ++d) {
                    if (d < D) {
                        if (vec) {
                            __builtin_nontemporal_store(f32x4{v[d][0] * rcp[0], v[d][1] * rcp[1], v[d][2] * rcp[2], v[d][3] * rcp[3]},
                                                        reinterpret_cast<f32x4*>(np + d * OHW));
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (e < nvalid) np[d * OHW + e] = v[d][e] * rcp[e];
                        }
                    }
                }
            }
        } else {
            float o[4];
            for (int d = 0; d < D; ++d) {
                blend4(d, o);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], o[e]);
            }
            for (int d = 0; d < D; ++d) {
                blend4(d, o);
                const float w = inv_idx[d];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ex = expf(o[e] - m[e]);
                    s[e] += ex;
                    t[e] = fmaf(ex, w, t[e]);
                }
            }
            if (np) {
                for (int d = 0; d < D; ++d) {
                    blend4(d, o);
                    if (vec) {
                        __builtin_nontemporal_store(f32x4{expf(o[0] - m[0]) / s[0], expf(o[1] - m[1]) / s[1], expf(o[2] - m[2]) / s[2],
                                                          expf(o[3] - m[3]) / s[3]}, reinterpret_cast<f32x4*>(np + d * OHW));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (e < nvalid) np[d * OHW + e] = expf(o[e] - m[e]) / s[e];
                    }
                }
            }
        }
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = t[e] / s[e];
            r[e] = post_div == 1.0f ? r[e] : r[e] / post_div;
        }
        if (vec) {
            *reinterpret_cast<f32x4*>(inv_dist + idx) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nvalid) inv_dist[idx + e] = r[e];
        }
    }
}

}  // namespace

extern "C" int mvsgi_softargmin_div_f32(const float* costs, const float* inv_idx, float* inv_dist, float* norm_costs,
                                        int B, int D, int H, int W, int scale, float post_div, mvsgi_stream_t stream);

extern "C" int mvsgi_softargmin_f32(const float* costs, const float* inv_idx, float* inv_dist, float* norm_costs,
                                    int B, int D, int H, int W, int scale, mvsgi_stream_t stream) {
    return mvsgi_softargmin_div_f32(costs, inv_idx, inv_dist, norm_costs, B, D, H, W, scale, 1.0f, stream);
}

extern "C" int mvsgi_softargmin_div_f32(const float* costs, const float* inv_idx, float* inv_dist, float* norm_costs,
                                        int B, int D, int H, int W, int scale, float post_div, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(costs && inv_idx && inv_dist, "mvsgi_softargmin_f32: null pointer");
    MVSGI_REQUIRE(post_div != 0.0f, "mvsgi_softargmin_div_f32: post_div must be non-zero");
    MVSGI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mvsgi_softargmin_f32: non-positive dimension");
    MVSGI_REQUIRE(scale == 1 || scale == 2, "mvsgi_softargmin_f32: scale %d not in {1, 2}", scale);
    if (scale == 2) {
        // row-pair kernel: column tiles of xt low-resolution columns (a multiple of 4), 2 * (xt / 2) threads, LDS 2 * D * (xt + 4) floats
        int xt = (int)(mvsgi::cdiv(W, 4) * 4);
        const int xt_max = (D > 16 && D <= 32) ? 512 : 640;      // = the kernels' launch bounds
        while ((xt > xt_max || (size_t)2 * D * (xt + 4) * 4 > 64 * 1024) && xt > 64) xt = (int)(mvsgi::cdiv(xt / 2, 4) * 4);
        // a frame or two: narrower column tiles until the launch has a workgroup or two per CU (one [16, 80, 320] frame: 81 workgroups
        // of 320 columns -> 324 of 80)
        while (xt > 64 && (long long)B * (H + 1) * mvsgi::cdiv(W, xt) < 2ll * mvsgi::device_cus()) xt = (int)(mvsgi::cdiv(xt / 2, 4) * 4);
        const size_t lds = (size_t)2 * D * (xt + 4) * 4;
        const long long xtiles = mvsgi::cdiv(W, xt), units = (long long)B * (H + 1) * xtiles;
        if (lds <= 160 * 1024 && units < (1ll << 31)) {
            const int threads = (int)(mvsgi::cdiv(xt, 64) * 64);          // 2 rows x xt / 2 pixels quads, whole waves
            auto kern = D <= 16 ? softargmin_rows_kernel<16> : (D <= 32 ? softargmin_rows_kernel<32> : softargmin_rows_kernel<0>);
            static bool attr_set[3][mvsgi::kMaxDevices] = {};
            int dev = 0;
            (void)hipGetDevice(&dev);
            const int ki = D <= 16 ? 0 : (D <= 32 ? 1 : 2);
            if (lds > 64 * 1024 && dev >= 0 && dev < mvsgi::kMaxDevices && !attr_set[ki][dev]) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                MVSGI_REQUIRE(e == hipSuccess, "mvsgi_softargmin_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
                attr_set[ki][dev] = true;
            }
            hipLaunchKernelGGL(kern, dim3((unsigned)units), dim3(threads), lds, mvsgi::as_stream(stream), costs, inv_idx, inv_dist,
                               norm_costs, B, D, H, W, xt, (int)xtiles, (int)units, post_div, 1);
            return mvsgi::check_launch("mvsgi_softargmin_f32(rows)");
        }
    }
    MVSGI_REQUIRE(H * scale < 65536 && B < 65536, "mvsgi_softargmin_f32: dimensions exceed the launch geometry");
    hipLaunchKernelGGL(softargmin_kernel, dim3((unsigned)mvsgi::cdiv(W * scale, 256), (unsigned)(H * scale), (unsigned)B), dim3(256), 0,
                       mvsgi::as_stream(stream), costs, inv_idx, inv_dist, norm_costs, B, D, H, W, scale, post_div);
    return mvsgi::check_launch("mvsgi_softargmin_f32");
}

// Any scale factor F.interpolate accepts.  1 and 2 forward to the launches above; integer factors >= 3 take the row-band
// kernel; everything else (fractional, down-scaling) takes the thread-per-pixel kernel, which is there for correctness, not
// speed.  variant: MVSGI_SA_AUTO, or MVSGI_SA_PIXEL | MVSGI_SA_BAND to force one of the two (tests, A/B timing).
extern "C" int mvsgi_softargmin_scaled_f32(const float* costs, const float* inv_idx, float* inv_dist, float* norm_costs,
                                           int B, int D, int H, int W, double scale, int OH, int OW, float post_div, int variant,
                                           mvsgi_stream_t stream) {
    MVSGI_REQUIRE(costs && inv_idx && inv_dist, "mvsgi_softargmin_scaled_f32: null pointer");
    MVSGI_REQUIRE(post_div != 0.0f, "mvsgi_softargmin_scaled_f32: post_div must be non-zero");
    MVSGI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mvsgi_softargmin_scaled_f32: non-positive dimension");
    MVSGI_REQUIRE(std::isfinite(scale) && scale > 0.0, "mvsgi_softargmin_scaled_f32: scale %g is not a finite positive factor", scale);
    MVSGI_REQUIRE(variant == MVSGI_SA_AUTO || variant == MVSGI_SA_PIXEL || variant == MVSGI_SA_BAND,
                  "mvsgi_softargmin_scaled_f32: unknown variant %d", variant);
    // F.interpolate: floor(in * scale) in double
    const double oh = std::floor((double)H * scale), ow = std::floor((double)W * scale);
    MVSGI_REQUIRE(oh >= 1.0 && ow >= 1.0, "mvsgi_softargmin_scaled_f32: scale %g gives an empty %g x %g output for %d x %d", scale, oh, ow, H, W);
    MVSGI_REQUIRE(oh < 65536.0 && ow < 2147483648.0 && B < 65536,
                  "mvsgi_softargmin_scaled_f32: output %g x %g (B = %d) exceeds the launch geometry", oh, ow, B);
    MVSGI_REQUIRE(OH == (int)oh && OW == (int)ow, "mvsgi_softargmin_scaled_f32: caller's output %d x %d is not floor(%d x %d * %g) = %d x %d",
                  OH, OW, H, W, scale, (int)oh, (int)ow);
    const bool integer = scale == std::floor(scale) && scale <= 64.0;
    if (variant == MVSGI_SA_AUTO && (scale == 1.0 || scale == 2.0))
        return mvsgi_softargmin_div_f32(costs, inv_idx, inv_dist, norm_costs, B, D, H, W, (int)scale, post_div, stream);
    MVSGI_REQUIRE(variant != MVSGI_SA_BAND || (integer && scale >= 3.0),
                  "mvsgi_softargmin_scaled_f32: the row-band kernel takes integer factors 3 .. 64, not %g", scale);
    const float rs = (float)(1.0 / scale);
    if (variant != MVSGI_SA_PIXEL && integer && scale >= 3.0) {
        // column tiles sized as for the row-pair kernel: LDS 2 * D * (xt + 4) floats, 64 KiB preferred; a frame or two:
        // narrower tiles until the launch has about two workgroups per CU
        int xt = (int)(mvsgi::cdiv(W, 4) * 4);
        while ((xt > 640 || (size_t)2 * D * (xt + 4) * 4 > 64 * 1024) && xt > 64) xt = (int)(mvsgi::cdiv(xt / 2, 4) * 4);
        while (xt > 64 && (long long)B * (H + 1) * mvsgi::cdiv(W, xt) < 2ll * mvsgi::device_cus()) xt = (int)(mvsgi::cdiv(xt / 2, 4) * 4);
        const size_t lds = (size_t)2 * D * (xt + 4) * 4;
        const long long xtiles = mvsgi::cdiv(W, xt), units = (long long)B * (H + 1) * xtiles;
        if (lds <= 160 * 1024 && units < (1ll << 31)) {
            const bool x4 = scale == 4.0;             // the product case has its own instances (compile-time taps)
            auto kern = x4 ? (D <= 16 ? softargmin_band_kernel<16, true> : (D <= 32 ? softargmin_band_kernel<32, true> : softargmin_band_kernel<0, true>))
                           : (D <= 16 ? softargmin_band_kernel<16, false> : (D <= 32 ? softargmin_band_kernel<32, false> : softargmin_band_kernel<0, false>));
            static bool attr_set[6][mvsgi::kMaxDevices] = {};
            int dev = 0;
            (void)hipGetDevice(&dev);
            const int ki = (x4 ? 3 : 0) + (D <= 16 ? 0 : (D <= 32 ? 1 : 2));
            if (lds > 64 * 1024 && dev >= 0 && dev < mvsgi::kMaxDevices && !attr_set[ki][dev]) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                MVSGI_REQUIRE(e == hipSuccess, "mvsgi_softargmin_scaled_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
                attr_set[ki][dev] = true;
            }
            hipLaunchKernelGGL(kern, dim3((unsigned)units), dim3(256), lds, mvsgi::as_stream(stream), costs, inv_idx, inv_dist,
                               norm_costs, B, D, H, W, (int)scale, rs, xt, (int)xtiles, (int)units, post_div);
            return mvsgi::check_launch("mvsgi_softargmin_scaled_f32(band)");
        }
        MVSGI_REQUIRE(variant != MVSGI_SA_BAND, "mvsgi_softargmin_scaled_f32: D = %d does not fit the row-band kernel's LDS", D);
    }
    hipLaunchKernelGGL(softargmin_scaled_kernel, dim3((unsigned)mvsgi::cdiv(OW, 256), (unsigned)OH, (unsigned)B), dim3(256), 0,
                       mvsgi::as_stream(stream), costs, inv_idx, inv_dist, norm_costs, B, D, H, W, OH, OW, rs, post_div);
    return mvsgi::check_launch("mvsgi_softargmin_scaled_f32");
}
